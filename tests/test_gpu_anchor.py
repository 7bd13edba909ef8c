"""The seam anchor term (anchor.hip, ast_set_anchor / ast_anchor_loss) -- run on an MI355X.

  anchor_b = mu sum_t w (a(x) - ref)^2 / sum_t w,   a = the TF inv_mu_law

against numpy float64 with oracle.astyle_oracle.inv_mu_law_tf.  Contexts as in test_gpu_stft.py:
taps [0] / [0], lambd = 0, targets the clips' own embeddings, so the content and style gradients
vanish and the term is isolated as grad(mu) - grad(unset).  Bars, the ones test_gpu_stft.py holds
for the same fp32 inv_mu_law value and derivative: value rel <= 1e-5, gradient rel-L2 <= 1e-4.
The term is computed in fp32 with fixed-order sums: a zero-weight clip, a cleared term, another
batch slot and a graph replay are all bit-exact statements."""
import numpy as np
import pytest
import torch

from oracle import astyle_oracle as O
from test_gpu_stft import _inputs, rel

pytestmark = pytest.mark.gpu

MU = 2.5
KW = dict(cont_ids=[0], style_ids=[0])


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda', 0)


def _engine(B, T, weights, precision='fp32', x=None):
    from audio_style_transfer_amd.engine import StyleEngine
    eng = StyleEngine(B, T, KW['cont_ids'], KW['style_ids'], lambd=0.0, precision=precision,
                      weights=weights)
    if x is not None:
        emb_c, emb_s = eng.embeds(x)
        eng.set_targets(emb_c.clone(), emb_s.clone())
    return eng


def _case(T, dev):
    B = 3
    x = _inputs(B, T, T).astype(np.float32)
    rng = np.random.default_rng(T + 1)
    ref = rng.uniform(-1, 1, (B, T)).astype(np.float32)
    w = np.zeros((B, T), np.float32)
    w[0, 37:421] = 1.0
    w[0, T - 300:T - 1] = 1.0
    w[1] = 1.0
    t = lambda a: torch.tensor(a, device=dev)
    return x, ref, w, t(x), t(ref), t(w)


def _oracle(x, ref, w, mu=MU):
    a, da = O.inv_mu_law_tf(x.astype(np.float64))
    sw = w.astype(np.float64).sum()
    if sw == 0:
        return 0.0, np.zeros_like(a)
    d = a - ref.astype(np.float64)
    return mu * (w * d * d).sum() / sw, 2 * mu * w * d * da / sw


@pytest.fixture(scope='module')
def runs(weights, dev):
    """Per T: the unset and the set evaluation of one B = 3 fp32 context, computed once."""
    out = {}
    for T in (512, 3584, 4096):
        x, ref, w, xt, rt, wt = _case(T, dev)
        eng = _engine(3, T, weights, 'fp32', xt)
        assert float(eng.anchor_loss().abs().sum()) == 0.0           # 0 while unset
        p0, g0 = eng.loss_grad(xt)
        p0, g0 = p0.clone(), g0.clone()
        eng.set_anchor(rt, wt, MU)
        p1, g1 = eng.loss_grad(xt)
        p1, g1 = p1.clone(), g1.clone()
        al = eng.anchor_loss()
        torch.cuda.synchronize()
        out[T] = dict(x=x, ref=ref, w=w, xt=xt, rt=rt, wt=wt, eng=eng, p0=p0, g0=g0, p1=p1, g1=g1, al=al)
    return out


@pytest.mark.parametrize('T', [512, 3584, 4096])
def test_value_and_gradient_match_fp64(T, runs):
    r = runs[T]
    p0, p1, al = r['p0'].cpu().numpy().astype(np.float64), r['p1'].cpu().numpy().astype(np.float64), r['al'].cpu().numpy()
    dg = (r['g1'] - r['g0']).cpu().numpy().astype(np.float64)
    for b in range(2):
        v, g = _oracle(r['x'][b], r['ref'][b], r['w'][b])
        # lambd = 0, gamma = 0: the other three weighted parts of the total are content alone
        from_parts = p1[b, 0] - p1[b, 1]
        e = rel(dg[b], g)
        print('T %d clip %d: anchor %.7g, from parts %.7g (fp64 %.7g), grad rel-L2 %.3g' % (T, b, al[b], from_parts, v, e))
        assert abs(al[b] - v) <= 1e-5 * v
        assert abs(from_parts - v) <= 1e-5 * v
        assert np.array_equal(p1[b, 1:], p0[b, 1:])
        assert e <= 1e-4


@pytest.mark.parametrize('T', [512, 3584, 4096])
def test_zero_weight_clip_is_untouched(T, runs):
    r = runs[T]
    assert torch.equal(r['g1'][2], r['g0'][2]) and torch.equal(r['p1'][2], r['p0'][2])
    assert float(r['al'][2]) == 0.0


@pytest.mark.parametrize('precision', ['fp32', 'split'])
def test_cleared_term_leaves_no_trace(precision, weights, dev):
    T = 4096
    x, ref, w, xt, rt, wt = _case(T, dev)
    never = _engine(3, T, weights, precision, xt)
    pn, gn = never.loss_grad(xt)
    eng = _engine(3, T, weights, precision, xt)
    eng.set_anchor(rt, wt, MU)
    p1, g1 = eng.loss_grad(xt)
    assert not torch.equal(g1, gn)
    gen = eng.gen
    eng.set_anchor(None)
    assert eng.gen > gen
    p2, g2 = eng.loss_grad(xt)
    assert torch.equal(g2, gn) and torch.equal(p2, pn)
    assert float(eng.anchor_loss().abs().sum()) == 0.0


@pytest.mark.parametrize('T', [512, 3584, 4096])
def test_slot_invariance(T, runs, weights, dev):
    r = runs[T]
    for b in range(3):
        xb = r['xt'][b:b + 1].contiguous()
        e1 = _engine(1, T, weights, 'fp32', xb)
        p0, g0 = e1.loss_grad(xb)
        p0, g0 = p0.clone(), g0.clone()
        e1.set_anchor(r['rt'][b:b + 1].contiguous(), r['wt'][b:b + 1].contiguous(), MU)
        p1, g1 = e1.loss_grad(xb)
        assert torch.equal(e1.anchor_loss()[0], r['al'][b])
        assert torch.equal(g1[0] - g0[0], r['g1'][b] - r['g0'][b])
        assert torch.equal(p1[0, 0] - p1[0, 1], r['p1'][b, 0] - r['p1'][b, 1])
    # ... and from run to run
    p, g = r['eng'].loss_grad(r['xt'])
    assert torch.equal(g, r['g1']) and torch.equal(p, r['p1'])


def test_graph_replay_follows_the_anchor(weights, dev):
    """An AdamLoop with the term set: replays equal eager steps bit for bit, a ref overwritten in
    place is picked up by the next replay, and setting the term after a capture is not ignored
    (after test_gamma_change_after_capture_is_not_ignored)."""
    from audio_style_transfer_amd.engine import AdamLoop
    T = 4096
    x, ref, w, xt, rt, wt = _case(T, dev)
    ref2 = torch.tensor(np.random.default_rng(5).uniform(-1, 1, ref.shape).astype(np.float32), device=dev)
    eng = _engine(3, T, weights, 'fp32', xt)
    outs = []
    for graph in (False, True):
        eng.set_anchor(None)
        rbuf = rt.clone()
        xx = xt.clone()
        loop = AdamLoop(eng, xx, lr=1.0, graph=graph)       # captured without the term
        vals = []
        for i in range(6):
            if i == 1:
                eng.set_anchor(rbuf, wt, MU)                # after the capture
            if i == 4:
                rbuf.copy_(ref2)                            # in place, no recapture
            p = loop.step()
            vals.append((p.clone(), eng.anchor_loss().clone()))
        torch.cuda.synchronize()
        outs.append((xx.clone(), vals))
    assert torch.equal(outs[0][0], outs[1][0])
    for (pe, ae), (pg, ag) in zip(outs[0][1], outs[1][1]):
        assert torch.equal(pe, pg) and torch.equal(ae, ag)
    a = [float(v[1][1]) for v in outs[1][1]]
    assert a[0] == 0.0 and a[1] > 0.0                       # the term came alive at step 1


def test_device_lbfgs_with_the_term(weights, dev):
    """T = 4096, one epoch, maxiter 5: in every history row the total is >= the sum of the other
    three weighted parts and differs from it, and the total decreases over accepted iterations."""
    from audio_style_transfer_amd.engine import LbfgsLoop
    T = 4096
    x, ref, w, xt, rt, wt = _case(T, dev)
    eng = _engine(3, T, weights, 'fp32', xt)
    eng.set_anchor(rt, wt, MU)
    loop = LbfgsLoop(eng, maxiter=5)
    loop.begin(xt.double())
    accepted, it = [[], [], []], np.zeros(3, int)
    for _ in range(200):
        loop.step()
        info, _ = loop.state()
        parts = loop.parts.cpu().numpy()
        for b in range(3):               # an iteration count that grew: this evaluation was accepted
            if info[b, 1] > it[b]:
                accepted[b].append(float(parts[b, 0]))
                it[b] = info[b, 1]
        if not info[:, 0].any():
            break
    assert not info[:, 0].any()
    hist = loop.history(info)
    for b in range(2):
        h = hist[b]
        assert len(h) >= 2 and len(accepted[b]) == info[b, 1] >= 1
        other = h[:, 1] + 0.0 * h[:, 2] + 0.0 * h[:, 3]      # lambd = 0, gamma = 0
        assert (h[:, 0] >= other).all() and (h[:, 0] - other != 0).all()
        tot = [h[0, 0]] + accepted[b]
        print('clip %d: totals over accepted iterations %s' % (b, tot))
        assert all(t1 < t0 for t0, t1 in zip(tot, tot[1:]))
