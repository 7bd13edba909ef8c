"""The inputs of tests/test_gpu_terms.py have teeth: conditions on the cases, from the fp64
oracle alone (no kernel runs here).

A gradient test at rel-L2 <= 2e-3 notices a lost or misplaced term only if that term carries
well over 2e-3 of the gradient.  For every balanced case (term_oracle.CASES, at its lambd*):
  * the content term and the style term each carry 0.3 .. 0.95 of |g|;
  * every content occurrence, and every distinct style tensor of a case with <= 5 style taps,
    carries >= 1e-2 of |g| (5x the gradient bar: losing it alone fails the GPU test);
  * lambd* is |g_content| / |g_style| of the first clip slot to one significant digit.
For every tap-focused case (term_oracle.focus_target) the content term is exactly zero and the
focused tap carries >= 0.4 of |g|.
A case that misses a condition is changed (taps, seeds, lambd*, phi_c_offset), not the floor.
"""
import numpy as np
import pytest

import term_oracle as TO
from oracle import astyle_oracle as O

SHARE_LO, SHARE_HI = 0.3, 0.95
TAP_FLOOR = 1e-2
FOCUS_FLOOR = 0.4


def test_terms_add_up_to_the_oracle_gradient(weights):
    """The helper against O.loss_and_grad: g_content + lambd g_style is the oracle's gradient,
    the occurrences add up to g_content and the style tensors to g_style."""
    case = TO.CASES['short']
    kw = TO.plan_kw(case)
    x, pc, ps = TO.case_problem(weights, case)
    t = TO.terms(x, weights, phi_c=pc, phi_s=ps, **kw)
    for lambd in (100.0, case['lam']):
        parts, g = O.loss_and_grad(x, weights, phi_c=pc, phi_s=ps, lambd=lambd, **kw)
        assert np.allclose(t.parts(lambd), parts[:3], rtol=1e-12, atol=0)
        assert TO.rel(t.grad(lambd), g) <= 1e-10
    occ = sum(t.occurrence(j) for j in range(len(kw['cont_ids'])))
    assert TO.rel(occ, t.g_content) <= 1e-10
    taps = sum(t.tap(k) for k in t.style_tensors())
    assert TO.rel(taps, t.g_style) <= 1e-10
    assert np.linalg.norm(t.g_content) > 0 and np.linalg.norm(t.g_style) > 0


def test_occurrences_of_a_repeated_and_a_bottleneck_tap(weights):
    """occurrence() with a repeated tap (both land on one extract) and the 16-wide bottleneck."""
    T = 512
    kw = dict(cont_ids=[3, 3, 31], style_ids=[29, 30, 2], gatys=True, nb_channels=128, cnt_channels=20)
    assert TO.content_columns(kw['cont_ids'], 20) == [(0, 20), (20, 40), (40, 56)]
    x = TO.clip(T)
    fwd = TO.forward(x, weights, **kw)
    rng = np.random.default_rng(0)
    pc = O.content_embeds(fwd[0], kw['cont_ids'], 20) + rng.normal(size=(T, 56))
    ps = O.l2_normalize(rng.normal(size=(3, 128, 128)))
    t = TO.terms(x, weights, phi_c=pc, phi_s=ps, fwd=fwd, **kw)
    occ = [t.occurrence(j) for j in range(3)]
    assert TO.rel(sum(occ), t.g_content) <= 1e-10
    assert TO.rel(occ[0], occ[1]) > 0.5            # their own phi_c columns, not one shared
    assert t.style_tensors() == [2, 29]            # 29 and 30 are one tensor
    assert TO.rel(t.tap(2) + t.tap(29), t.g_style) <= 1e-10


def test_masked_oracle_gatys_and_bottleneck(weights):
    """oracle/masked_oracle.py with the Gatys Gram and a bottleneck content tap: on its own relu
    pattern it is O.loss_and_grad, and forcing one decision the other way moves the gradient."""
    from oracle import masked_oracle as M
    T = 512
    kw = dict(cont_ids=[3, 31], style_ids=[29, 30, 2], gatys=True, nb_channels=128, cnt_channels=20)
    x = TO.clip(T)
    rng = np.random.default_rng(1)
    pc = rng.normal(size=(T, 36))
    ps = O.l2_normalize(rng.normal(size=(3, 128, 128)))
    parts, g = O.loss_and_grad(x, weights, phi_c=pc, phi_s=ps, lambd=3e4, **kw)
    mparts, mg, ext, masks = M.loss_and_grad(x, weights, phi_c=pc, phi_s=ps, lambd=3e4, **kw)
    assert np.allclose(mparts[:3], parts[:3], rtol=1e-12, atol=0) and TO.rel(mg, g) <= 1e-12
    assert len(ext) == 32 and ext[31].shape == (T, 16)
    me = [m.copy() for m in masks[0]]
    me[7][100, 5] ^= True
    _, g2, _, _ = M.loss_and_grad(x, weights, phi_c=pc, phi_s=ps, lambd=3e4, me=me, mu=masks[1], **kw)
    assert TO.rel(g2, g) > 0


@pytest.mark.parametrize('name', list(TO.CASES))
def test_balanced_case_has_teeth(name, weights):
    case = TO.CASES[name]
    kw = TO.plan_kw(case)
    for slot in range(len(case['seeds'])):
        x, pc, ps = TO.case_problem(weights, case, slot)
        t = TO.terms(x, weights, phi_c=pc, phi_s=ps, **kw)
        lam = case['lam']
        ratio = np.linalg.norm(t.g_content) / np.linalg.norm(t.g_style)
        c, s = TO.shares(t, lam)
        n = np.linalg.norm(t.grad(lam))
        occ = [float(np.linalg.norm(t.occurrence(j)) / n) for j in range(len(kw['cont_ids']))]
        taps = {}
        if len(kw['style_ids']) <= 5:
            taps = {k: float(lam * np.linalg.norm(t.tap(k)) / n) for k in t.style_tensors()}
        print('%s slot %d: |g_c|/|g_s| %.4g lambd* %g shares content %.3f style %.3f occurrences %s '
              'style tensors %s' % (name, slot, ratio, lam, c, s, ['%.3g' % v for v in occ],
                                    {k: '%.3g' % v for k, v in taps.items()}))
        if slot == 0:
            assert TO.one_digit(ratio) == lam, (ratio, lam)
        assert SHARE_LO <= c <= SHARE_HI and SHARE_LO <= s <= SHARE_HI, (slot, c, s)
        assert min(occ) >= TAP_FLOOR, (slot, occ)
        assert not taps or min(taps.values()) >= TAP_FLOOR, (slot, taps)


def _clips():
    """{(T, content seed, noise seed): blocks}: every clip of the cases, with the most blocks a
    case runs on it."""
    out = {(TO.FOCUS_T, 1000, 380): 30}
    for case in TO.CASES.values():
        for sc, _, sn in case['seeds']:
            key = (case['T'], sc, sn)
            out[key] = max(out.get(key, 0), O.needed_blocks(case['cont_ids'], case['style_ids']))
    return out


@pytest.mark.parametrize('T,seed,noise', list(_clips()))
def test_clip_has_no_relu_tie_below_the_formats_resolution(T, seed, noise, weights):
    """A decision closer to zero than 2^-22 of its layer's max (split mode's 22 significant bits;
    fp32: 2^-24) falls either way in a correct run and is worth up to 5e-3 of a balanced gradient
    (term_oracle.FORMAT_RESOLUTION).  mu_law(clip 1000) + default_rng(8).normal(0, 4) at T = 1024
    has one at 3.4e-9 (u_7[459, 34]), worth 3.0e-3 of 'bott_only' and 4.0e-3 of the ours tap-0
    case; with noise seed 12 three between 6.6e-8 and 1.3e-7, together 6.8e-3 of the ours tap-29
    case.  Clips of T <= 1024 have none; for 3584 samples the closest is printed."""
    _, cache = O.encoder_forward(TO.clip(T, seed, noise), weights, _clips()[(T, seed, noise)])
    r = TO.closest_tie(cache)
    print('clip T=%d seeds %d/%d: closest relu tie %.3g of the layer max' % (T, seed, noise, r))
    assert T > 1024 or r > TO.FORMAT_RESOLUTION, r


_FWD = {}


def _focus_fwd(weights):
    if 'fwd' not in _FWD:
        _FWD['fwd'] = TO.forward(TO.clip(TO.FOCUS_T), weights, cont_ids=[29], style_ids=TO.ALL30)
    return _FWD['fwd']


@pytest.mark.parametrize('gatys', [False, True], ids=['ours', 'gatys'])
@pytest.mark.parametrize('k', TO.FOCUS_TAPS)
def test_focused_tap_carries_the_gradient(k, gatys, weights):
    fwd = _focus_fwd(weights)
    pc, ps = TO.focus_target(fwd, k, gatys)
    kw = dict(cont_ids=[29], style_ids=TO.ALL30, gatys=gatys, nb_channels=128, cnt_channels=128)
    t = TO.terms(None, weights, phi_c=pc, phi_s=ps, fwd=fwd, **kw)
    assert t.content == 0.0 and not t.g_content.any()
    share = float(np.linalg.norm(t.tap(k)) / np.linalg.norm(t.g_style))
    print('focus %s k=%d: tap share %.3f style part %.4g' % ('gatys' if gatys else 'ours', k, share, t.style))
    assert share >= FOCUS_FLOOR, share
