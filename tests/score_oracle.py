"""numpy oracle of decoder scoring (helper module, no tests): the sequence form of
decoder_oracle.sequence_run with a selectable input table, and the log-likelihood of the bins it
is teacher-forced on.

  input_mode 0   x_s = xs256[bin], the synthesis feedback table (decoder_oracle.tables)
  input_mode 1   x_s = (bin - 128) / 128, the training graph (nsynth/wavenet/model.py:213-214, 264)

Built from decoder_oracle's _causal_conv / _condition; for the xs256 table it asserts equality with
decoder_oracle.sequence_run.  Runs in any float dtype: float64 is the reference, float32 the
yardstick of the tolerances.  Also a numpy stand-in for synthesis.Decoder's scoring interface.
"""
import numpy as np

import decoder_oracle as O

NBIN = 256


def input_table(input_mode):
    """bin -> the scaled input x_s, float32 [256]."""
    if input_mode == 0:
        return O.tables()[1]
    if input_mode == 1:
        return ((np.arange(NBIN) - 128) / 128.0).astype(np.float32)
    raise ValueError('input_mode %r' % (input_mode,))


def sequence_logits(W, enc, n_layers, n_stages, hop, bins, input_mode=0, dtype=np.float64):
    """Logits [B, T, 256] of the decoder teacher-forced on ``bins`` [B, T], T <= R hop."""
    W = O._cast(W, dtype)
    enc = np.asarray(enc, dtype=dtype)
    width = W['startconv/W'].shape[3]
    x = input_table(input_mode)[np.asarray(bins)].astype(dtype)[:, :, None]
    x = np.concatenate([np.zeros_like(x[:, :1]), x[:, :-1]], axis=1)      # masked.shift_right
    l = O._causal_conv(x, W['startconv/W'], W['startconv/biases'], 1)
    s = l @ W['skip_start/W'][0, 0] + W['skip_start/biases']
    for i in range(n_layers):
        k = i + 1
        a = O._causal_conv(l, W['dilatedconv_%d/W' % k], W['dilatedconv_%d/biases' % k], 2 ** (i % n_stages))
        a = O._condition(a, enc @ W['cond_map_%d/W' % k][0, 0] + W['cond_map_%d/biases' % k], hop)
        d = 1.0 / (1.0 + np.exp(-a[..., :width])) * np.tanh(a[..., width:])
        l = l + d @ W['res_%d/W' % k][0, 0] + W['res_%d/biases' % k]
        s = s + d @ W['skip_%d/W' % k][0, 0] + W['skip_%d/biases' % k]
    s = np.maximum(s, 0)
    s = s @ W['out1/W'][0, 0] + W['out1/biases']
    s = np.maximum(O._condition(s, enc @ W['cond_map_out1/W'][0, 0] + W['cond_map_out1/biases'], hop), 0)
    return s @ W['logits/W'][0, 0] + W['logits/biases']


def score(W, enc, n_layers, n_stages, hop, bins, input_mode=0, dtype=np.float64):
    """dict(logits, pmf [B, T, 256], logp [B, T], nll [B]) in ``dtype``."""
    bins = np.asarray(bins)
    logits = sequence_logits(W, enc, n_layers, n_stages, hop, bins, input_mode, dtype)
    if input_mode == 0:
        ref = O.sequence_run(W, enc, n_layers, n_stages, hop, bins, dtype=dtype)
        assert np.array_equal(ref['logits'], logits)
    mx = logits.max(axis=-1, keepdims=True)
    e = np.exp(logits - mx)
    den = e.sum(axis=-1, keepdims=True, dtype=dtype)
    lab = np.take_along_axis(logits - mx, bins[..., None].astype(np.int64), axis=-1)[..., 0]
    logp = (lab - np.log(den[..., 0])).astype(dtype)
    return dict(logits=logits, pmf=e / den, logp=logp, nll=(-logp.mean(axis=1, dtype=dtype)).astype(dtype))


def yardstick(W, enc, n_layers, n_stages, hop, bins, input_mode=0):
    """(float64 result, e32 = rel-L2 of the float32 logits, a32 = max |logp32 - logp64|)."""
    r64 = score(W, enc, n_layers, n_stages, hop, bins, input_mode, np.float64)
    r32 = score(W, enc, n_layers, n_stages, hop, bins, input_mode, np.float32)
    e32 = O.rel_l2(r32['logits'], r64['logits'])
    a32 = float(np.abs(r32['logp'].astype(np.float64) - r64['logp']).max())
    return r64, e32, a32


class NumpyScorer(object):
    """A stand-in for synthesis.Decoder on the CPU with its scoring interface (float32)."""

    calls = []      # (bins, enc, input_mode) of every score call, for the tests to inspect

    def __init__(self, batch, weights, device=None, width=512, skip_width=256, n_layers=30,
                 n_stages=10, hop=512, graph_steps=16):
        self.W = weights
        self.n_layers, self.n_stages, self.hop = n_layers, n_stages, hop
        self.closed = False

    def score(self, bins, enc, input_mode=0, want_pmf=False, want_logits=False):
        NumpyScorer.calls.append((np.array(bins), np.array(enc), input_mode))
        r = score(self.W, enc, self.n_layers, self.n_stages, self.hop, bins, input_mode, np.float32)
        out = dict(logp=r['logp'], nll=r['nll'], bits=r['nll'] / np.float32(np.log(2.0)))
        if want_pmf:
            out['pmf'] = r['pmf']
        if want_logits:
            out['logits'] = r['logits']
        return out

    def close(self):
        self.closed = True
