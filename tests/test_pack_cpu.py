"""CPU: the weight-fragment packing of csrc/pack.h, the contract every bf16 and split-fp16 block
kernel reads its weights by, byte for byte against the index formulas of pack.h's comment
restated in numpy; and the knob reader of csrc/knob.h (a value outside a knob's domain is the
default).  Both through the stand-alone host driver tests/san/fuzz_driver.cpp (`pack`, `knob`).

Every packed quantity is exactly representable (a power-of-two scaling, one fp16 rounding, an
fp32 difference of two values that agree to 11 bits, one more fp16 rounding; one bf16 rounding),
so the comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

C = 128
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1:abort_on_error=0',
           UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')


@pytest.fixture(scope='module')
def driver():
    import san.build as SB
    return SB.build()


def _run(driver, *args):
    r = subprocess.run([driver, *args], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
    return r.stdout


def _frag_index(m16):
    """(kk, mm - 32 w) of slot kb, lane, element e, each [8][64][8]"""
    kb, ln, e = np.ogrid[:8, :64, :8]
    if m16:
        kk, mm = 32 * (kb >> 1) + 8 * (ln >> 4) + e, 16 * (kb & 1) + (ln & 15) + 0 * e
    else:
        kk, mm = 16 * kb + 8 * (ln >> 5) + e, (ln & 31) + 0 * kb + 0 * e
    return np.broadcast_to(kk, (8, 64, 8)), np.broadcast_to(mm, (8, 64, 8))


def _elems(W, bwd, kk, mm):
    """[4 w][taps][8 kb][64 lanes][8]: W[tap][kk][32 w + mm] (forward) or W[tap][32 w + mm][kk]"""
    w = np.arange(4)[:, None, None, None, None]
    tp = np.arange(W.shape[0])[None, :, None, None, None]
    K, M = kk[None, None], 32 * w + mm[None, None]
    return W[tp, M, K] if bwd else W[tp, K, M]


def _ref_split(W, bwd, m16):
    k = 14 - int(np.frexp(np.abs(W).max())[1])
    v = np.ldexp(_elems(W, bwd, *_frag_index(m16)), k).astype(np.float32)
    hi = v.astype(np.float16)                              # round to nearest
    lo = (v - hi.astype(np.float32)).astype(np.float16)    # the fp32 difference, rounded
    return k, np.ascontiguousarray(np.stack([hi, lo], axis=3)).view(np.uint16)   # [4][taps][8][2 hl][64][8]


def _bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)   # round to nearest even


def _ref_bf16(W, bwd):
    kk, mm = _frag_index(False)
    if W.shape[0] == 1 and not bwd:   # forward W_r: K in kperm(kb, lane >> 5, e) order
        s, ln, e = np.ogrid[:8, :64, :8]
        kk = 32 * (s >> 1) + 16 * (s & 1) + (e & 3) + 8 * (e >> 2) + 4 * (ln >> 5)
    return _bf16(_elems(W, bwd, kk, mm).transpose(1, 0, 2, 3, 4))     # [taps][4 w][8][64][8]


def test_fragments_match_the_layout_formulas(driver, tmp_path):
    out = str(tmp_path / 'pack.bin')
    _run(driver, 'pack', '11', out)
    raw = open(out, 'rb').read()
    os.remove(out)
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(raw, dtype=dtype, count=n, offset=pos)
        pos += a.nbytes
        return a

    exps = set()
    for case in range(3):     # as drawn, x 1e-4, x 1e3
        w = take(np.float32, 4 * C * C)
        Ws = {'W_d': w[:3 * C * C].reshape(3, C, C), 'W_r': w[3 * C * C:].reshape(1, C, C)}
        assert np.isfinite(w).all() and np.abs(w).max() > 0
        for name, W in Ws.items():
            for m16 in (False, True):
                for bwd in (False, True):
                    k = int(take(np.int32, 1)[0])
                    got = take(np.uint16, W.size * 2)
                    rk, ref = _ref_split(W, bwd, m16)
                    assert k == rk, (case, name, m16, bwd, k, rk)
                    top = float(np.abs(np.ldexp(W.astype(np.float64), k)).max())
                    assert 2.0 ** 13 <= top < 2.0 ** 14, (case, name, k, top)
                    assert got.tobytes() == ref.tobytes(), (case, name, 'split', m16, bwd)
                    exps.add((name, k))
        for name, W in Ws.items():
            for bwd in (False, True):
                got = take(np.uint16, W.size)
                assert got.tobytes() == _ref_bf16(W, bwd).tobytes(), (case, name, 'bf16', bwd)
    assert pos == len(raw)
    assert len({k for n, k in exps if n == 'W_d'}) == 3 and len({k for n, k in exps if n == 'W_r'}) == 3


def test_knob_outside_its_domain_is_the_default(driver):
    # e.g. ASTYLE_GRAM_FWDN_NC takes 4 or 8: 2 (which would size a grid the kernels do not
    # decode) is as unset
    assert _run(driver, 'knob').split() == ['0']
