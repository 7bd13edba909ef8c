"""GPU: decoder scoring (ast_dec_score, synthesis.Decoder.score) against the numpy oracle
(score_oracle.py), its bit-exact statements, the step path on the device, and its errors.

Configurations are those of test_gpu_decoder.py: S = width 64, skip 32, 4 layers, 2 stages, hop 8;
SP = S with logits/W x 8 (a peaked pmf); M = width 512, skip 256, 11 layers, 10 stages, hop 512;
F = the full default network.

The yardstick of the tolerances is the oracle's own float32 run against its float64 run on the same
inputs: e32 = rel-L2 of the float32 logits, a32 = max |logp32 - logp64|.  The device's pmf must be
within max(4 e32, 1e-6) rel-L2 of the float64 pmf, its logp within 4 a32 max abs of the float64
logp, and nll within 2e-6 relative of -mean(logp_dev) taken in float64.
"""
import numpy as np
import pytest
import torch

import decoder_oracle as O
import score_oracle as SO
from audio_style_transfer_amd import _lib
from test_gpu_decoder import CFG, enc_of, make_decoder, weights_of

pytestmark = pytest.mark.gpu

_REF = {}


def bins_of(batch, T, seed=5):
    return np.random.RandomState(seed).randint(0, 256, size=(batch, T))


def net(name):
    c = CFG[name]
    return c['n_layers'], c['n_stages'], c['hop']


def reference(name, batch, T, mode):
    """(enc, bins, float64 result, e32, a32), computed once per case and left unchanged."""
    key = (name, batch, T, mode)
    if key not in _REF:
        c = CFG[name]
        R = -(-T // c['hop'])
        enc = np.random.RandomState(100).randn(batch, R, 16).astype(np.float32)
        bins = bins_of(batch, T)
        _REF[key] = (enc, bins) + SO.yardstick(weights_of(name), enc, *net(name), bins, mode)
    return _REF[key]


def device_score(name, bins, enc, mode=0, **kw):
    dec = make_decoder(name, batch=1)        # the score batch is independent of the context's
    try:
        return dec.score(bins, enc, input_mode=mode, **kw)
    finally:
        dec.close()


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('name,batch,T', [('S', 3, 40), ('S', 3, 37), ('SP', 1, 40), ('M', 2, 1100), ('F', 1, 64)])
def test_accuracy_against_the_float64_oracle(name, batch, T, mode):
    """Check 1.  Measured on MI355X (the test prints them; the two input tables are equal in
    float32, so both modes measure the same), e32 / device pmf rel-L2 against float64 / the bar
    max(4 e32, 1e-6) | a32 / device logp max abs against float64 / the bar 4 a32 | nll relative to
    -mean(logp_dev) in float64 (bar 2e-6):
      S  T 40    1.55e-7 / 3.15e-7 / 1e-6     | 7.29e-7 / 1.07e-6 / 2.92e-6 | 3.1e-8
      S  T 37    1.56e-7 / 3.06e-7 / 1e-6     | 6.76e-7 / 9.63e-7 / 2.70e-6 | 3.7e-8
      SP T 40    1.57e-7 / 6.57e-7 / 1e-6     | 4.24e-6 / 4.56e-6 / 1.69e-5 | 3.5e-9   (max pmf 0.985)
      M  T 1100  4.48e-7 / 7.27e-7 / 1.79e-6  | 1.89e-6 / 2.40e-6 / 7.57e-6 | 2.8e-8
      F  T 64    6.73e-7 / 1.27e-6 / 2.69e-6  | 3.26e-6 / 4.36e-6 / 1.30e-5 | 3.2e-8
    The 4 a32 bar is not degenerate on any of them.  DESIGN.md 7f holds the same table."""
    enc, bins, r64, e32, a32 = reference(name, batch, T, mode)
    got = device_score(name, bins, enc, mode, want_pmf=True, want_logits=True)
    assert got['logp'].shape == (batch, T) and got['nll'].shape == (batch,)
    err = O.rel_l2(got['pmf'], r64['pmf'])
    elog = O.rel_l2(got['logits'], r64['logits'])
    bar = max(4 * e32, 1e-6)
    aerr = float(np.abs(got['logp'].astype(np.float64) - r64['logp']).max())
    mean64 = -got['logp'].astype(np.float64).mean(axis=1)
    nerr = float(np.abs(got['nll'].astype(np.float64) - mean64).max() / np.abs(mean64).min())
    print('%s B %d T %d mode %d: e32 %.3g | pmf rel-L2 %.3g logits rel-L2 %.3g (bar %.3g) | a32 %.3g logp max abs %.3g '
          '(bar %.3g) | nll rel %.3g | nll64 %s max pmf %.3g'
          % (name, batch, T, mode, e32, err, elog, bar, a32, aerr, 4 * a32, nerr, r64['nll'], r64['pmf'].max()))
    assert err <= bar, (err, bar)
    assert aerr <= 4 * a32, (aerr, 4 * a32)
    assert nerr <= 2e-6, nerr
    assert (got['bits'] == got['nll'] / np.float32(np.log(2.0))).all()
    assert np.abs(got['pmf'].astype(np.float64).sum(-1) - 1).max() < 1e-5


def test_a_clip_is_bit_identical_alone_and_in_any_slot():
    """Check 2: each clip of the S batch-3 run equals its batch-1 run; run to run."""
    enc, bins, _, _, _ = reference('S', 3, 40, 0)
    b3 = device_score('S', bins, enc, want_pmf=True)
    again = device_score('S', bins, enc, want_pmf=True)
    for k in ('logp', 'pmf', 'nll'):
        assert (b3[k] == again[k]).all(), k
    perm = device_score('S', bins[[2, 0, 1]], enc[[2, 0, 1]], want_pmf=True)
    for slot, clip in enumerate([2, 0, 1]):
        one = device_score('S', bins[[clip]], enc[[clip]], want_pmf=True)
        for k in ('logp', 'pmf', 'nll'):
            assert (one[k][0] == b3[k][clip]).all(), (k, clip)
            assert (one[k][0] == perm[k][slot]).all(), (k, slot)
    assert len({b3['logp'][i].tobytes() for i in range(3)}) == 3      # the clips do differ


@pytest.mark.parametrize('name,batch,T,Tp', [('S', 3, 40, 23), ('M', 2, 1100, 1030)])
def test_a_prefix_run_equals_the_first_columns(name, batch, T, Tp):
    """Check 2: the network is causal and a column's arithmetic does not depend on T."""
    enc, bins, _, _, _ = reference(name, batch, T, 0)
    whole = device_score(name, bins, enc, want_pmf=True)
    part = device_score(name, bins[:, :Tp], enc, want_pmf=True)
    assert (part['logp'] == whole['logp'][:, :Tp]).all()
    assert (part['pmf'] == whole['pmf'][:, :Tp]).all()


def test_eager_equals_a_graph_replayed_twice():
    """Check 2: ast_dec_score is launches only; canaries after the outputs stay."""
    enc, bins, _, _, _ = reference('S', 3, 37, 0)
    dec = make_decoder('S', batch=1)
    try:
        eager = dec.score(bins, enc, want_pmf=True)
        st = dec._score_buffers(3, 37, want_pmf=True)
        st['bins'].copy_(torch.as_tensor(bins.astype(np.int32)))
        enc_dev = torch.as_tensor(enc, device=dec.device)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            dec._score_launch(st, enc_dev, enc.shape[1], 0)
        for _ in range(2):
            for k in ('logp', 'nll', 'pmf'):
                st[k].fill_(7.5)
            g.replay()
            torch.cuda.synchronize()
            for k in ('logp', 'nll', 'pmf'):
                assert (st[k].cpu().numpy() == eager[k]).all(), k
    finally:
        dec.close()


def test_score_equals_the_step_path_teacher_forced():
    """Check 3: the full network, 1 clip, 2100 samples.  Both paths are fp32 sums of the same
    products in different orders, each within max(4 e32_F, 1e-6) of float64, so they are within
    twice that of each other; e32_F is the oracle's at F (64 samples).  Also logp against
    log(pmf[label]), bar 1e-6.  Measured on MI355X: e32_F 6.73e-7, score pmf against step pmf
    rel-L2 2.03e-6 (bar 5.38e-6), logp against log(pmf[label]) 8.87e-7 max abs."""
    T = 2100
    _, _, _, e32_F, _ = reference('F', 1, 64, 0)
    bar = 2 * max(4 * e32_F, 1e-6)
    R = -(-T // CFG['F']['hop'])
    enc = np.random.RandomState(104).randn(1, R, 16).astype(np.float32)
    bins = bins_of(1, T, seed=6)
    dec = make_decoder('F', batch=1)
    try:
        dec.start(enc, np.full((1, T), 0.5, np.float32), force=bins, want_pmf=True)
        assert dec.run() == T
        step_pmf = dec.pmf()
        got = dec.score(bins, enc, input_mode=0, want_pmf=True)
    finally:
        dec.close()
    gap = O.rel_l2(got['pmf'], step_pmf)
    lab = np.take_along_axis(got['pmf'].astype(np.float64), bins[..., None], axis=2)[..., 0]
    lerr = float(np.abs(got['logp'].astype(np.float64) - np.log(lab)).max())
    print('F T %d: e32_F %.3g | score pmf against step pmf rel-L2 %.3g (bar %.3g) | logp - log pmf[label] max abs %.3g'
          % (T, e32_F, gap, bar, lerr))
    assert gap <= bar, (gap, bar)
    assert lerr <= 1e-6, lerr


def test_a_score_call_does_not_disturb_a_synthesis():
    """Check 4: 40 steps of S with a score call after step 16 equal the uninterrupted run."""
    B, total = 3, 40
    enc = enc_of('S', B, seed=3)
    u = np.random.RandomState(23).rand(B, total).astype(np.float32)
    sb, senc = bins_of(2, 40, seed=8), enc_of('S', 2, seed=5)
    dec = make_decoder('S', batch=B)
    try:
        dec.start(enc, u, want_pmf=True)
        assert dec.run() == total
        plain = dict(bins=dec.bins(), pmf=dec.pmf())
        alone = dec.score(sb, senc, want_pmf=True)
        dec.start(enc, u, want_pmf=True)
        assert dec.run(16) == 16
        mid = dec.score(sb, senc, want_pmf=True)
        assert dec.run() == total
        assert (dec.bins() == plain['bins']).all() and (dec.pmf() == plain['pmf']).all()
        assert (mid['logp'] == alone['logp']).all() and (mid['pmf'] == alone['pmf']).all()
    finally:
        dec.close()


def test_bad_arguments_are_refused_before_any_launch():
    """Check 5."""
    lib = _lib.load()
    dec = make_decoder('S', batch=1)
    try:
        dev = dec.device
        B, R, T = 2, 5, 40
        st = dec._score_buffers(B, T)
        st['bins'].zero_()
        enc = torch.zeros(B, R, 16, device=dev)
        st['logp'].fill_(7.5)
        st['nll'].fill_(7.5)

        def call(T=T, mode=0, work_bytes=st['need'], logp=st['logp'], batch=B):
            rc = lib.ast_dec_score(dec.h, dec._p(st['bins']), dec._p(enc), batch, R, T, mode, dec._p(st['work']),
                                   work_bytes, dec._p(logp), dec._p(st['nll']), None, None, dec._stream())
            return rc, lib.ast_last_error().decode()

        for kw, word in ((dict(T=0), 'T 0'), (dict(T=R * 8 + 1), 'T 41'), (dict(work_bytes=st['need'] - 1), 'work_bytes'),
                         (dict(mode=2), 'input_mode'), (dict(logp=None), 'null'), (dict(batch=0), 'batch')):
            rc, msg = call(**kw)
            assert rc == -1 and word in msg, (kw, rc, msg)
        torch.cuda.synchronize()
        assert (st['logp'] == 7.5).all() and (st['nll'] == 7.5).all()
        rc, msg = call()
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert (st['logp'] < 0).all()
        for bad in (np.full((1, 8), 256), np.full((1, 8), -1)):
            with pytest.raises(_lib.AstError, match='0..255'):
                dec.score(bad, np.zeros((1, 1, 16), np.float32))
        with pytest.raises(_lib.AstError, match='exceeds'):
            dec.score(np.zeros((1, 9), np.int64), np.zeros((1, 1, 16), np.float32))
    finally:
        dec.close()
