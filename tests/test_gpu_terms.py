"""The content and the style gradient held to the fp64 oracle term by term — run on an MI355X.

The other gradient tests compare the total d loss / d x at lambd = 100, where the content term
carries almost all of it (the whole Gatys style term is 3e-4 .. 1e-3 of |g|, under the 2e-3 bar:
a Gram backward that wrote zeros would pass them).  Here:
  A  the fused plans (cont 29, style 0..29, ours and Gatys, T = 1024 and 3584) at a lambd* that
     gives each term 0.65 .. 0.82 of |g|;
  B  one style tap at a time with the content term exactly zero (phi_c = the engine's own
     embedding of x): taps 0, 9, 10, 19, 20, 29 of the 30, ours and Gatys;
  C  the tap-plan branches of plan() / fused_content_occ() / loss_grad_front() (api.hip), each at
     its lambd*, three of them with two different clips and per-clip targets.
tests/test_terms_cpu.py holds, from the oracle alone, that every term, content occurrence and
style tensor these cases are about carries at least 5x the gradient bar.

Bars are the project's own (test_gpu_parity.py, test_gpu_split.py): fp32 and split loss parts
rel <= 1e-4 and gradient rel-L2 <= 2e-3; bf16 gradient cosine >= 0.98 and rel-L2 <= 0.25.  A
fp32 / split gradient above 2e-3 is separated as in test_gpu_precision.py (the oracle forced onto
the run's relu pattern): it passes only with arithmetic <= 2e-3, every differing relu decision
a near-tie (|fp64 value| <= 1e-6 max |layer|) and the total within 1e-3 per such flip.

The clips of T <= 1024 have no relu decision closer to zero than the formats under test resolve
(2^-22 of the layer's max, term_oracle.FORMAT_RESOLUTION, held by tests/test_terms_cpu.py): one
such flip is worth up to 5e-3 of these gradients, so with them a correct run measured up to
6.8e-3.  Without them fp32 and split take every decision as the oracle does, and the figures
below are arithmetic alone.

Measured on an MI355X (gradient rel-L2, fp32 / split / bf16; content / style share of |g|):
  fused29     3.5e-6 / 3.3e-5 / 0.166   0.72 / 0.73      above      3.8e-6 / 3.2e-5 / 0.090
  ours_odd    8.4e-4 / 2.1e-3 / 0.165   0.75 / 0.69      dupstyle   3.9e-6 / 3.4e-5 / 0.168
  gatys_fused 3.7e-6 / 3.2e-5 / 0.098   0.73 / 0.70      cont_twice 3.2e-6 / 2.7e-5 / 0.151
  gatys_odd   4.6e-4 / 1.4e-3 / 0.109   0.74 / 0.72      cnt3       8.0e-6 / 6.0e-5 / 0.166
  nb1         3.8e-6 / 3.8e-5 / 0.174   0.72 / 0.71      nb100      3.8e-6 / 3.3e-5 / 0.160
  short       9.5e-7 / 5.8e-6 / 0.046   0.64 / 0.83      bott_only  5.0e-6 / 3.6e-5 / 0.145
  alias30     3.6e-6 / 3.3e-5 / 0.169   0.69 / 0.73      gatys_dup  3.7e-6 / 3.4e-5 / 0.110
  second clip slots (B = 2): cnt3 7.5e-6 / 6.1e-5 / 0.165, nb100 4.1e-6 / 3.4e-5 / 0.137,
  gatys_dup 3.9e-6 / 3.6e-5 / 0.104; the first slots bit for bit as at B = 1.
  one tap alone, fp32 / split, k = 0, 9, 10, 19, 20, 29:
    ours   3.2e-5 / 2.5e-4, 1.2e-5 / 9.4e-5, 8.8e-6 / 6.9e-5, 4.5e-6 / 3.5e-5, 3.8e-6 / 3.0e-5,
           2.5e-6 / 1.5e-5
    gatys  2.3e-5 / 2.7e-4, 1.0e-5 / 1.2e-4, 1.1e-5 / 1.3e-4, 1.5e-5 / 1.7e-4, 1.6e-5 / 1.8e-4,
           1.9e-5 / 2.2e-4
The 3584-sample clip (ours_odd, gatys_odd) has about twenty such decisions at any seed: ours_odd
in split mode is 2.1e-3 = arithmetic 4.2e-4 plus ten flips of <= 2.4e-7 of their layer's max, held
by the separation above.
"""
import numpy as np
import pytest
import torch

import term_oracle as TO
from oracle import astyle_oracle as O
from oracle import masked_oracle as M

pytestmark = pytest.mark.gpu

PART_BAR = 1e-4
GRAD_BAR = 2e-3
FLIP_ALLOWANCE = 1e-3      # per near-tie relu flip, as tests/test_gpu_precision.py
BF16_COS, BF16_REL = 0.98, 0.25

A_CASES = ['fused29', 'ours_odd', 'gatys_fused', 'gatys_odd']
C_CASES = ['above', 'dupstyle', 'cont_twice', 'cnt3', 'nb1', 'nb100', 'short', 'bott_only',
           'alias30', 'gatys_dup']
TWO_CLIP_CASES = [n for n in C_CASES if len(TO.CASES[n]['seeds']) == 2]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda', 0)


_REF = {}


def _ref(name, slot, weights):
    """One oracle evaluation per case and clip slot, shared by the precisions."""
    key = (name, slot)
    if key not in _REF:
        case = TO.CASES[name]
        x, pc, ps = TO.case_problem(weights, case, slot)
        t = TO.terms(x, weights, phi_c=pc, phi_s=ps, **case)
        _REF[key] = dict(x=x, phi_c=pc, phi_s=ps, parts=t.parts(case['lam']), grad=t.grad(case['lam']),
                         shares=TO.shares(t, case['lam']))
    return _REF[key]


def _engine(B, T, kw, lambd, precision, weights, dev):
    from audio_style_transfer_amd.engine import StyleEngine
    return StyleEngine(B, T, kw['cont_ids'], kw['style_ids'], cnt_channels=kw['cnt_channels'],
                       nb_channels=kw['nb_channels'], gatys=kw['gatys'], lambd=lambd,
                       weights=weights, precision=precision, device=dev)


def _separate(eng, xt, b, x, kw, phi_c, phi_s, lambd, weights, g):
    """(arithmetic error, [near-tie ratio of every relu decision the run took differently])."""
    nb = O.needed_blocks(kw['cont_ids'], kw['style_ids'])
    eng.forward(xt)
    ext = [eng.extract(i).cpu().numpy()[b] for i in range(nb - 1)]
    mh = M.masks_from_extracts(x, weights, ext, n_blocks=nb)
    _, gm, _, _ = M.loss_and_grad(x, weights, phi_c=phi_c, phi_s=phi_s, lambd=lambd, me=mh[0],
                                  mu=mh[1], **kw)
    _, cache, m64 = M.forward(x, weights, nb)
    ties = []
    for kind, k in (('e', 0), ('u', 1)):
        for l in range(nb):
            ref = cache['es' if kind == 'e' else 'us'][l]
            for t, c in np.argwhere(mh[k][l] != m64[k][l]):
                ties.append((kind, l, int(t), int(c), float(abs(ref[t, c]) / np.abs(ref).max())))
    return M.rel(g, gm), ties


def _hold(tag, precision, parts, grad, ref_parts, ref_grad, separate=None):
    parts = np.asarray(parts, np.float64)
    g = np.asarray(grad, np.float64)
    e = TO.rel(g, ref_grad)
    cos = float(np.dot(g, ref_grad) / max(np.linalg.norm(g) * np.linalg.norm(ref_grad), 1e-300))
    perr = [abs(parts[k] - ref_parts[k]) / max(abs(ref_parts[k]), 1e-30) for k in range(3)]
    print('TERMS %s %s: grad rel-L2 %.3e cosine %.6f parts rel %s' % (tag, precision, e, cos, ['%.1e' % v for v in perr]))
    assert np.isfinite(parts).all() and np.isfinite(g).all()
    if precision == 'bf16':
        assert cos >= BF16_COS and e <= BF16_REL, (cos, e)
        return
    for k in range(3):
        assert abs(parts[k] - ref_parts[k]) <= PART_BAR * abs(ref_parts[k]) + 1e-7, (k, parts, ref_parts)
    if e <= GRAD_BAR:
        return
    assert separate is not None, e
    arith, ties = separate(g)
    print('TERMS %s %s: above the bar: arithmetic %.3e flips %s' % (tag, precision, arith, ties))
    assert arith <= GRAD_BAR, (arith, e)
    assert all(r <= 1e-6 for *_, r in ties), ties
    assert e <= GRAD_BAR + FLIP_ALLOWANCE * len(ties), (e, arith, ties)


def _run_case(name, precision, slots, weights, dev):
    case = TO.CASES[name]
    kw = TO.plan_kw(case)
    refs = [_ref(name, s, weights) for s in slots]
    B = len(refs)
    eng = _engine(B, case['T'], kw, case['lam'], precision, weights, dev)
    try:
        if B == 1:      # shared targets
            pc, ps = torch.tensor(refs[0]['phi_c'], dtype=torch.float32), torch.tensor(refs[0]['phi_s'], dtype=torch.float32)
        else:           # per-clip targets, all different
            pc = torch.tensor(np.stack([r['phi_c'] for r in refs]), dtype=torch.float32)
            ps = torch.tensor(np.stack([r['phi_s'] for r in refs]), dtype=torch.float32)
        eng.set_targets(pc, ps)
        xt = torch.tensor(np.stack([r['x'] for r in refs]), dtype=torch.float32, device=dev)
        parts, grad = eng.loss_grad(xt)
        parts, grad = parts.cpu().numpy(), grad.cpu().numpy()
        for b, r in enumerate(refs):
            tag = '%s[B=%d slot %d] shares %.2f/%.2f' % ((name, B, slots[b]) + r['shares'])
            _hold(tag, precision, parts[b], grad[b], r['parts'], r['grad'],
                  lambda g, b=b, r=r: _separate(eng, xt, b, r['x'], kw, r['phi_c'], r['phi_s'],
                                                case['lam'], weights, g))
    finally:
        eng.close()


@pytest.mark.parametrize('precision', ['fp32', 'split', 'bf16'])
@pytest.mark.parametrize('name', A_CASES)
def test_balanced_terms(name, precision, weights, dev):
    """A: each term carries 0.65 .. 0.82 of |g|, so a lost or badly scaled Gram backward (ours or
    Gatys, with the content tap fused in in split mode) misses the bar."""
    _run_case(name, precision, [0], weights, dev)


@pytest.mark.parametrize('precision', ['fp32', 'split', 'bf16'])
@pytest.mark.parametrize('name', C_CASES)
def test_tap_plan_branches(name, precision, weights, dev):
    """C: a content tap above every style tap (the chain starts from a content-gradient buffer,
    launch_absmax), repeated / aliased style taps in ours mode (lmap not the identity), a repeated
    content tap (accumulate), a content width that is no multiple of 4 with extract 0, the
    bottleneck and a direct tap together, nb_channels 1 and 100, T = 512 with 4 blocks, content
    through the bottleneck alone, content on extract 30 with style on 29, and the Gatys
    duplicate-tap plan in split mode."""
    _run_case(name, precision, [0], weights, dev)


@pytest.mark.parametrize('precision', ['fp32', 'split', 'bf16'])
@pytest.mark.parametrize('name', TWO_CLIP_CASES)
def test_two_clips_with_their_own_targets(name, precision, weights, dev):
    """Two different clips, each with its own phi_c and phi_s (phi_bstride = nb L L with nb = 100,
    L L C C in Gatys mode, cont_phi_bstride / phi_bstride = T ncc with ncc = 9): each slot against
    its own oracle evaluation."""
    _run_case(name, precision, [0, 1], weights, dev)


_FOCUS = {}


def _focus_ref(k, gatys, weights):
    if 'fwd' not in _FOCUS:
        _FOCUS['x'] = TO.clip(TO.FOCUS_T)
        _FOCUS['fwd'] = TO.forward(_FOCUS['x'], weights, cont_ids=[29], style_ids=TO.ALL30)
    key = (k, gatys)
    if key not in _FOCUS:
        pc, ps = TO.focus_target(_FOCUS['fwd'], k, gatys)
        t = TO.terms(None, weights, phi_c=pc, phi_s=ps, fwd=_FOCUS['fwd'], cont_ids=[29],
                     style_ids=TO.ALL30, gatys=gatys, nb_channels=128, cnt_channels=128)
        assert t.content == 0.0
        _FOCUS[key] = dict(phi_c=pc, phi_s=ps, style=t.style, g_style=t.g_style,
                           share=float(np.linalg.norm(t.tap(k)) / np.linalg.norm(t.g_style)))
    return _FOCUS['x'], _FOCUS[key]


@pytest.mark.parametrize('precision', ['fp32', 'split'])
@pytest.mark.parametrize('gatys', [False, True], ids=['ours', 'gatys'])
@pytest.mark.parametrize('k', TO.FOCUS_TAPS)
def test_one_style_tap_alone(k, gatys, precision, weights, dev):
    """B: the style term alone, carried by one of the 30 taps.  phi_c is the engine's own content
    embedding of x, so the content part is exactly 0 and the gradient is lambd g_style; phi_s is
    x's own normalised Gram moved in row and column k (ours) or in matrix k (Gatys) only, so tap
    k carries 0.65 .. 1.0 of the gradient: a D that is lost, scaled wrong or lands on another
    tensor misses the bar.  Measured: see the module docstring."""
    lambd = TO.FOCUS_LAMBDA
    x, r = _focus_ref(k, gatys, weights)
    kw = dict(cont_ids=[29], style_ids=TO.ALL30, gatys=gatys, nb_channels=128, cnt_channels=128)
    eng = _engine(1, TO.FOCUS_T, kw, lambd, precision, weights, dev)
    try:
        xt = torch.tensor(x[None], dtype=torch.float32, device=dev)
        emb_c, _ = eng.embeds(xt, style=False)
        eng.set_targets(emb_c, torch.tensor(r['phi_s'], dtype=torch.float32))
        parts, grad = eng.loss_grad(xt)
        parts, grad = parts.cpu().numpy()[0], grad.cpu().numpy()[0]
        assert parts[1] == 0.0, parts
        ref_parts = np.array([lambd * r['style'], 0.0, r['style']])
        tag = 'focus %s k=%d tap share %.2f' % ('gatys' if gatys else 'ours', k, r['share'])
        _hold(tag, precision, parts, grad, ref_parts, lambd * r['g_style'],
              lambda g: _separate(eng, xt, 0, x, kw, r['phi_c'], r['phi_s'], lambd, weights, g))
    finally:
        eng.close()
