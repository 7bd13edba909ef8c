"""The NSynth encoding on the device (encpool.hip; ast_encoding, ast_set_encoding_target,
ast_encoding_loss; model.py:121-128, fastgen.py:86-113) -- run on an MI355X.

  enc(x)[b, r, j] = (1/512) sum_{t in hop r} (sum_c e_30[b, t, c] W_b[c, j] + b_b[j]),  R = T / 512
  enc_term_b      = omega mean_{r, j} (enc(x)[b, r, j] - phi_e[b, r, j])^2

against the fp64 oracle: encoder_forward(..., need_bottleneck=True), extract 31 reshaped to
[R, 512, 16] and averaged; the term's gradient is encoder_backward(cache, W, {31: g}) with
g[t, j] = 2 omega d[t // 512, j] / (16 R 512).

Bars.  Both come from the path this replaces, measured in the same process against the same
oracle, never from the code under test (``parent``): a cont=[31] context on the same input and
precision gives (a) avg_pool1d(extract(31)), whose rel-L2 error e_f is the forward yardstick, and
(b) its loss gradient with phi_c = the other clips' extract 31 (lambd = 0, so the gradient is the
extract-31 content gradient alone), whose rel-L2 error e_g is the gradient yardstick.
  * forward:  rel-L2 <= max(2 e_f, 1e-6) in fp32 and split, <= 2 e_f in bf16 (the kernel sums in
    another order but does no less precise arithmetic).
  * gradient: rel-L2 of grad(term set) - grad(term cleared) <= 2 e_g.  The content and style
    targets are the clips' own embeddings there, so the other gradients vanish and the difference
    is the term's alone (as test_gpu_stft.py / test_gpu_anchor.py isolate theirs).
  * value:    d = enc - phi_e with phi_e an exact input, so an encoding error of rel-L2 bar_f moves
    d by bar_f |enc| / |d| and the term, quadratic in d, by twice that (plus second order):
    rel <= 2.5 bar_f |enc| / |d_b| + 1e-5 per clip b (|enc| over the three clips, which bounds a
    clip's share of the error; 1e-5 for the fp32 sums of 16 R squares).
Everything else is a bit-exact statement: zero residual, another batch slot, another run, graph
replay, D in or out of place.

Measured on an MI355X (rel-L2; new / parent path, the bar is 2 x parent): see DESIGN.md §7d."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import astyle_oracle as O
from audio_style_transfer_amd.weights import synthetic_clips, synthetic_weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OMEGA = 5.0
TAPS = {'top': ([29], list(range(30))),      # tensor 30 is style-tapped (and content-tapped)
        'low': ([25], list(range(10)))}      # stack 0, content 25: tensor 30 carries the term alone
DEV = 'cuda:0'


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def inputs(T):
    """Three clips that differ (other sinusoids, other levels), in mu-law units."""
    clips = synthetic_clips(3, T, 1000) * np.array([[1.0], [0.45], [0.15]], np.float32)
    return O.mu_law_numpy(clips).astype(np.float32)


_ORACLE, _PARENT, _TERM = {}, {}, {}


def oracle(W, T):
    """Per T, once: the fp64 encodings [3, R, 16] and the encoder caches of the three clips."""
    if T not in _ORACLE:
        x = inputs(T)
        enc, caches = [], []
        for b in range(3):
            ext, cache = O.encoder_forward(x[b], W, need_bottleneck=True)
            enc.append(ext[31].reshape(T // 512, 512, 16).mean(1))
            caches.append(cache)
        _ORACLE[T] = (x, np.stack(enc), caches)
    return _ORACLE[T]


def engine(W, B, T, precision, taps='low', gatys=False, encoding=True, **kw):
    from audio_style_transfer_amd.engine import StyleEngine
    cont, sty = TAPS[taps] if isinstance(taps, str) else taps
    return StyleEngine(B, T, cont, sty, gatys=bool(gatys), precision=precision, weights=W,
                       encoding=encoding, **kw)


def parent(W, precision, T):
    """The yardsticks (e_f, e_g) of the module docstring, from a cont=[31] context without the
    encoding: what the project computed before this kernel existed."""
    key = (precision, T)
    if key not in _PARENT:
        x, enc64, _ = oracle(W, T)
        xt = torch.tensor(x, device=DEV)
        eng = engine(W, 3, T, precision, ([31], [0]), encoding=False, lambd=0.0)
        eng.forward(xt)
        e31 = eng.extract(31)
        pooled = torch.nn.functional.avg_pool1d(e31.transpose(1, 2), 512, 512).transpose(1, 2)
        e_f = rel(pooled.cpu().numpy(), enc64)
        emb_c, emb_s = eng.embeds(xt)
        phi_c = emb_c.roll(1, 0).contiguous()
        eng.set_targets(phi_c, emb_s.clone())
        _, g = eng.loss_grad(xt)
        pc = phi_c.cpu().numpy().astype(np.float64)
        ps = emb_s.cpu().numpy().astype(np.float64)
        g64 = np.stack([O.loss_and_grad(x[b].astype(np.float64), W, cont_ids=[31], style_ids=[0],
                                        phi_c=pc[b], phi_s=ps[b], lambd=0.0)[1] for b in range(3)])
        e_g = rel(g.cpu().numpy(), g64)
        eng.close()
        _PARENT[key] = (e_f, e_g)
    return _PARENT[key]


def fwd_bar(W, precision, T):
    e_f = parent(W, precision, T)[0]
    return 2 * e_f if precision == 'bf16' else max(2 * e_f, 1e-6)


def term_run(W, precision, gatys, taps, T):
    """One B = 3 with_encoding context, phi_e = the encodings of the other clips: numpy results of
    the evaluations the tests below read, computed once per configuration (and, with
    ASTYLE_DOOP=0, by test_d_in_place_equals_out_of_place's child process)."""
    key = (precision, gatys, taps, T)
    if key in _TERM:
        return _TERM[key]
    x = inputs(T)
    xt = torch.tensor(x, device=DEV)
    eng = engine(W, 3, T, precision, taps, gatys)
    n = lambda t: t.cpu().numpy().copy()
    enc = eng.encoding(xt)
    phi_e = enc.roll(1, 0).contiguous()
    emb_c, emb_s = eng.embeds(xt)
    out = dict(enc=n(enc), phi_e=n(phi_e), doop=eng.d_out_of_place())
    for name, tc, ts in (('self', emb_c.clone(), emb_s.clone()),
                         ('other', emb_c.roll(1, 0).contiguous(), emb_s.roll(1, 0).contiguous())):
        eng.set_targets(tc, ts)
        eng.set_encoding_target(None)
        p0, g0 = eng.loss_grad(xt)
        out[name + '_p0'], out[name + '_g0'], out[name + '_el0'] = n(p0), n(g0), n(eng.encoding_loss())
        eng.set_encoding_target(phi_e, OMEGA)
        p1, g1 = eng.loss_grad(xt)
        out[name + '_p1'], out[name + '_g1'], out[name + '_el'] = n(p1), n(g1), n(eng.encoding_loss())
        p2, g2 = eng.loss_grad(xt)                       # ... and from run to run
        out[name + '_again'] = bool(torch.equal(p1, p2) and torch.equal(g1, g2))
        # zero residual: the target is this input's own encoding
        eng.set_encoding_target(enc, OMEGA)
        pz, gz = eng.loss_grad(xt)
        out[name + '_pz'], out[name + '_gz'], out[name + '_elz'] = n(pz), n(gz), n(eng.encoding_loss())
    eng.close()
    _TERM[key] = out
    return out


# ------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize('T', [512, 1024, 1536])
@pytest.mark.parametrize('precision', ['fp32', 'split', 'bf16'])
def test_encoding_matches_fp64(precision, T, weights):
    x, enc64, _ = oracle(weights, T)
    e_f = parent(weights, precision, T)[0]
    eng = engine(weights, 3, T, precision)
    enc = eng.encoding(torch.tensor(x, device=DEV))
    assert enc.shape == (3, T // 512, 16)
    e = rel(enc.cpu().numpy(), enc64)
    eng.close()
    print('forward %s T %d: rel-L2 new %.3g, avg_pool1d(extract 31) %.3g' % (precision, T, e, e_f))
    assert e <= fwd_bar(weights, precision, T)


# --------------------------------------------------------------------- 2. term and gradient
CASES = [(p, g, t, 1024) for p in ('fp32', 'split', 'bf16') for g in (0, 1) for t in ('top', 'low')]
CASES += [('split', 0, 'top', 512), ('split', 0, 'low', 1536), ('bf16', 0, 'low', 1536), ('fp32', 1, 'top', 1536)]


@pytest.mark.parametrize('precision,gatys,taps,T', CASES)
def test_term_and_gradient_match_fp64(precision, gatys, taps, T, weights):
    x, enc64, caches = oracle(weights, T)
    e_f, e_g = parent(weights, precision, T)
    r = term_run(weights, precision, gatys, taps, T)
    R = T // 512
    d64 = enc64 - r['phi_e'].astype(np.float64)
    val64 = OMEGA * (d64 ** 2).mean(axis=(1, 2))
    g64 = np.stack([O.encoder_backward(caches[b], weights,
                                       {31: np.repeat(2 * OMEGA * d64[b] / (16 * R * 512), 512, axis=0)})
                    for b in range(3)])
    # value, against fp64 (both target sets evaluate the same term)
    # (a clip's encoding error is at most the three clips' together: bar_f |enc|)
    bar_v = 2.5 * fwd_bar(weights, precision, T) * np.linalg.norm(enc64) / np.sqrt((d64 ** 2).sum(axis=(1, 2))) + 1e-5
    e_v = np.abs(r['self_el'] - val64) / val64
    # gradient: own content / style targets, so grad(set) - grad(cleared) is the term's alone
    e = rel(r['self_g1'].astype(np.float64) - r['self_g0'], g64)
    print('term %s gatys %d taps %s T %d: value rel %s (bars %s); gradient rel-L2 %.3g, '
          'cont=[31] gradient %.3g; |grad cleared| / |grad term| %.3g'
          % (precision, gatys, taps, T, ' '.join('%.3g' % v for v in e_v),
             ' '.join('%.3g' % v for v in bar_v), e, e_g,
             np.linalg.norm(r['self_g0']) / np.linalg.norm(g64)))
    assert np.all(e_v <= bar_v)
    assert np.array_equal(r['self_el'], r['other_el'])
    assert e <= 2 * e_g
    # parts: the [B, 4] layout stays; the term enters the total alone, after the other three
    for name in ('self', 'other'):
        p0, p1, el = r[name + '_p0'], r[name + '_p1'], r[name + '_el']
        assert not r[name + '_el0'].any()                       # 0 while cleared
        assert np.array_equal(p1[:, 1:], p0[:, 1:])
        assert np.array_equal(p1[:, 0], (p0[:, 0] + el).astype(np.float32))
        weighted = p1[:, 1].astype(np.float64) + 100.0 * p1[:, 2] + 0.0 * p1[:, 3]
        assert np.all(np.abs(p1[:, 0] - (weighted + el)) <= 4e-7 * np.abs(p1[:, 0]))
        assert np.all(el > 0)
    assert np.linalg.norm(r['other_g0']) > 0                    # (the other targets do pull)


# ------------------------------------------------------------------------- 3. zero residual
@pytest.mark.parametrize('precision,gatys,taps,T', CASES)
def test_zero_residual_leaves_no_trace(precision, gatys, taps, T, weights):
    r = term_run(weights, precision, gatys, taps, T)
    for name in ('self', 'other'):
        assert not r[name + '_elz'].any()
        assert np.array_equal(r[name + '_gz'], r[name + '_g0'])
        assert np.array_equal(r[name + '_pz'], r[name + '_p0'])
        assert np.isfinite(r[name + '_g1']).all()


# ---------------------------------------------------------------------------- 4. invariance
@pytest.mark.parametrize('precision,gatys,taps,T', [('fp32', 0, 'low', 1024), ('split', 0, 'top', 1024),
                                                    ('bf16', 1, 'low', 1536), ('split', 1, 'low', 512)])
def test_slot_and_run_invariance(precision, gatys, taps, T, weights):
    r = term_run(weights, precision, gatys, taps, T)
    assert r['self_again'] and r['other_again']                 # two runs are bit-equal
    x = inputs(T)
    for b in range(3):
        xb = torch.tensor(x[b:b + 1], device=DEV)
        e1 = engine(weights, 1, T, precision, taps, gatys)
        assert np.array_equal(e1.encoding(xb).cpu().numpy()[0], r['enc'][b])
        emb_c, emb_s = e1.embeds(xb)
        e1.set_targets(emb_c.clone(), emb_s.clone())
        e1.set_encoding_target(torch.tensor(r['phi_e'][b:b + 1], device=DEV), OMEGA)
        p, g = e1.loss_grad(xb)
        assert np.array_equal(e1.encoding_loss().cpu().numpy()[0], r['self_el'][b])
        assert np.array_equal(g.cpu().numpy()[0], r['self_g1'][b])
        assert np.array_equal(p.cpu().numpy()[0], r['self_p1'][b])
        e1.close()


def test_shared_target(weights):
    """phi_e [R, 16] is one target for every clip."""
    T = 1024
    xt = torch.tensor(inputs(T), device=DEV)
    eng = engine(weights, 3, T, 'split')
    emb_c, emb_s = eng.embeds(xt)
    eng.set_targets(emb_c.clone(), emb_s.clone())
    phi = eng.encoding(xt)[2].contiguous()
    eng.set_encoding_target(phi, OMEGA)
    p1, g1 = (t.clone() for t in eng.loss_grad(xt))
    el1 = eng.encoding_loss().clone()
    eng.set_encoding_target(phi[None].repeat(3, 1, 1).contiguous(), OMEGA)
    p2, g2 = eng.loss_grad(xt)
    assert torch.equal(p1, p2) and torch.equal(g1, g2) and torch.equal(el1, eng.encoding_loss())
    assert float(el1[2]) == 0.0 and float(el1[0]) > 0.0
    eng.close()


def test_graph_replay_follows_the_target(weights):
    """An AdamLoop with the term set: three replays equal three eager steps bit for bit; phi_e
    overwritten in place is picked up by the next replay without a recapture."""
    from audio_style_transfer_amd.engine import AdamLoop
    T = 1024
    xt = torch.tensor(inputs(T), device=DEV)
    eng = engine(weights, 3, T, 'split', 'low')
    emb_c, emb_s = eng.embeds(xt)
    eng.set_targets(emb_c.roll(1, 0).contiguous(), emb_s.roll(1, 0).contiguous())
    enc = eng.encoding(xt)
    phi_a, phi_b = enc.roll(1, 0).contiguous(), (enc.roll(2, 0) * 1.5).contiguous()
    runs = {}
    for name, graph, overwrite in (('eager', False, True), ('graph', True, True), ('kept', True, False)):
        buf = phi_a.clone()
        eng.set_encoding_target(buf, OMEGA)
        xx = xt.clone()
        loop = AdamLoop(eng, xx, lr=1.0, graph=graph)
        g0, gen = loop.graph, eng.gen
        vals = []
        for i in range(5):
            if i == 3 and overwrite:
                buf.copy_(phi_b)                                # in place, no recapture
            p = loop.step()
            vals.append((p.clone(), eng.encoding_loss().clone()))
        torch.cuda.synchronize()
        assert loop.graph is g0 and eng.gen == gen
        runs[name] = (xx.clone(), vals)
    assert torch.equal(runs['eager'][0], runs['graph'][0])
    for (pe, le), (pg, lg) in zip(runs['eager'][1], runs['graph'][1]):
        assert torch.equal(pe, pg) and torch.equal(le, lg)
    for i in range(5):                                          # the overwrite took effect at step 3
        same = torch.equal(runs['graph'][1][i][1], runs['kept'][1][i][1])
        assert same == (i < 3), i
    eng.close()


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_encoding as M
W = M.synthetic_weights(0)
out = {}
for gatys in (0, 1):
    for taps in ('top', 'low'):
        r = M.term_run(W, 'split', gatys, taps, 1024)
        for k in ('doop', 'enc', 'other_p1', 'other_g1', 'other_el', 'other_gz', 'self_g1'):
            out['%d%s_%s' % (gatys, taps, k)] = r[k]
np.savez(sys.argv[2], **out)
'''


def test_d_in_place_equals_out_of_place(tmp_path, weights):
    """The contexts of this file keep D out of place (the default where it fits); a child process
    with ASTYLE_DOOP=0 (read once per process) runs the same evaluations with D in place over the
    activations: the same bits, ours and Gatys, tensor 30 style-tapped or not."""
    f = str(tmp_path / 'inplace.npz')
    r = subprocess.run([sys.executable, '-c', CHILD, ROOT, f], env=dict(os.environ, ASTYLE_DOOP='0'),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(f)
    for gatys in (0, 1):
        for taps in ('top', 'low'):
            here = term_run(weights, 'split', gatys, taps, 1024)
            k0 = '%d%s_' % (gatys, taps)
            assert here['doop'] and not z[k0 + 'doop']
            for k in ('enc', 'other_p1', 'other_g1', 'other_el', 'other_gz', 'self_g1'):
                assert np.array_equal(z[k0 + k], here[k]), (gatys, taps, k)


# --------------------------------------------------------------------------- 5. off means off
def test_context_without_encoding_refuses(weights):
    from audio_style_transfer_amd import _lib
    T = 512
    eng = engine(weights, 1, T, 'fp32', encoding=False)
    xt = torch.tensor(inputs(T)[:1], device=DEV)
    buf = torch.zeros(1, 1, 16, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert eng.lib.ast_encoding(eng.h, p(xt), p(buf), None) == -3              # AST_E_STATE
    assert b'with_encoding' in eng.lib.ast_last_error()
    assert eng.lib.ast_set_encoding_target(eng.h, p(buf), 0, 1.0) == -3
    assert eng.lib.ast_encoding_loss(eng.h, p(buf), None) == -3
    with pytest.raises(_lib.AstError):
        eng.encoding(xt)
    with pytest.raises(_lib.AstError):
        eng.set_encoding_target(buf, 1.0)
    eng.close()
    # ... and a with_encoding context refuses a negative or non-finite omega
    eng = engine(weights, 1, T, 'fp32')
    for bad in (-1.0, float('inf'), float('nan')):
        assert eng.lib.ast_set_encoding_target(eng.h, p(buf), 0, bad) == -1     # AST_E_ARG
    eng.close()


# ---------------------------------------------------------------------- 6. CLI end to end
def _write(path, sig, sr=16000):
    from scipy.io import wavfile
    wavfile.write(path, sr, (sig * 32767).astype(np.int16))


def test_methods_cli_with_enc(tmp_path, weights, monkeypatch):
    """methods.main --enc 5 --optimizer device --epochs 1 (T = 4096, stack 0): writes ep-0.wav; in
    the loss history the total is the three weighted parts plus the term (at the first
    evaluation, x = 1e-6, the term an engine of its own gives); --enc 0 is the run without the
    flag, bit for bit."""
    from audio_style_transfer_amd import methods
    sr, T = 16000, 4096
    src = tmp_path / 'src'
    src.mkdir()
    _write(str(src / 'c.wav'), synthetic_clips(1, 3 * sr, 1000)[0])
    _write(str(src / 's.wav'), synthetic_clips(1, 3 * sr, 5000)[0])
    np.savez(str(tmp_path / 'w.npz'), **weights)
    nets = []

    class Rec(methods.GatysNet):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            nets.append(self)

    monkeypatch.setattr(methods, 'GatysNet', Rec)

    def run(tag, *extra):
        argv = ['c', 's', '--epochs', '1', '--batch_size', str(T), '--stack', '0', '--optimizer', 'device',
                '--dir', str(src), '--outdir', str(tmp_path / tag), '--logdir', str(tmp_path / (tag + 'log')),
                '--weights', str(tmp_path / 'w.npz'), '--no_plots', '--lambd', '100', '--gamma', '0.1']
        audio = methods.main(argv + list(extra))
        net = nets[-1]
        assert os.path.isfile(os.path.join(net.savepath, 'ep-0.wav'))
        return audio, np.array(net.history), net

    a5, h5, net = run('enc5', '--enc', '5')
    assert net.engine.with_encoding and 'enc' not in os.path.basename(net.savepath)
    assert np.all(np.isfinite(a5)) and len(h5) >= 2
    other = h5[:, 1] + 100.0 * h5[:, 2] + 0.1 * h5[:, 3]
    term = h5[:, 0] - other
    assert np.all(term > 0)
    # the first evaluation's term from a context of its own: encoding(x0) against phi_e
    eng = engine(weights, 1, T, 'split', ([29], list(range(10))))
    x0 = torch.full((1, T), 1e-6, device=DEV)
    want = 5.0 * float(((eng.encoding(x0)[0].cpu().double() - torch.tensor(net.phi_e, dtype=torch.float64)) ** 2).mean())
    eng.close()
    print('first evaluation: total %.7g, other parts %.7g, term %.7g (own context %.7g)'
          % (h5[0, 0], other[0], term[0], want))
    assert abs(term[0] - want) <= 1e-5 * want + 4e-7 * abs(h5[0, 0])
    a0, h0, net0 = run('enc0', '--enc', '0')
    an, hn, netn = run('none')
    assert not net0.engine.with_encoding and not netn.engine.with_encoding
    assert np.array_equal(a0, an) and np.array_equal(h0, hn)
    assert not np.array_equal(a5, an)
