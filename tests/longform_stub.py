"""CPU stand-in engine for the long-form CLI's tests (tests/test_longform.py): bench_stub's
StubEngine plus the seam anchor surface (set_anchor / anchor_loss) and a module-level stitch, so
``--engine longform_stub:AnchorStubEngine`` runs audio_style_transfer_amd.longform without a GPU.
The anchor term is the real one, mu * sum w (a(x) - ref)^2 / sum w per clip with a = inv_mu_law,
added to parts[:, 0] and the gradient.  Every minimize call's anchor state is appended to
longform_stub.LOG (None while the term is unset, else copies of ref and w and mu), and every
set_anchor call to longform_stub.CALLS, for the tests to read after an in-process run."""
from __future__ import annotations

import numpy as np
import torch

from audio_style_transfer_amd import longform
from bench_stub import IllCondStubEngine, LbfgsLoop, StubEngine  # noqa: F401  (LbfgsLoop: the module's loop)

DEVICE = 'cpu'


def _inv_mu_law(x):
    o = (x + 0.5) * (2.0 / 256.0)
    a = torch.sign(o) / 255.0 * (256.0 ** o.abs() - 1.0)
    da = np.log(256.0) * 256.0 ** o.abs() / 255.0 * (2.0 / 256.0)
    return torch.where(x == 0, x, a), torch.where(x == 0, torch.ones_like(x), da)


LOG = []      # per minimize call: None or (ref copy, w copy, mu)
CALLS = []    # per set_anchor call: 'set' or 'clear'


class _Anchor:

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._anchor = None

    def set_anchor(self, ref, w=None, mu=0.0):
        if ref is None or float(mu) == 0.0:
            self._anchor = None
            CALLS.append('clear')
        else:
            assert ref.shape == (self.batch, self.T) and w.shape == (self.batch, self.T)
            self._anchor = (ref, w, float(mu))
            CALLS.append('set')

    def _anchor_terms(self, x):
        ref, w, mu = self._anchor
        a, da = _inv_mu_law(x)
        sw = w.sum(1)
        ok = sw > 0
        den = torch.where(ok, sw, torch.ones_like(sw))
        val = torch.where(ok, mu * (w * (a - ref) ** 2).sum(1) / den, torch.zeros_like(sw))
        g = 2.0 * mu * w * (a - ref) * da / den[:, None] * ok[:, None]
        return val, g

    def loss_grad(self, x, grad=None, parts=None):
        parts, grad = super().loss_grad(x, grad, parts)
        self._last = torch.zeros(self.batch)
        if self._anchor is not None:
            val, g = self._anchor_terms(x)
            parts[:, 0] += val
            grad += g
            self._last = val
        return parts, grad

    def anchor_loss(self):
        return getattr(self, '_last', torch.zeros(self.batch)).clone()

    def end_minimize(self, active):
        a = self._anchor
        LOG.append(None if a is None else (a[0].clone(), a[1].clone(), a[2]))
        if hasattr(super(), 'end_minimize'):
            super().end_minimize(active)


class AnchorStubEngine(_Anchor, StubEngine):
    pass


class IllCondAnchorStubEngine(_Anchor, IllCondStubEngine):
    """The ill-conditioned problem: windows keep running over epochs, so later epochs (and with
    --seam the anchor term) are reached."""


def stitch(x, late, fade):
    """engine.stitch's interface over longform.stitch_numpy."""
    n, T = x.shape
    geo = longform.geometry(T, fade, n)
    assert geo.late == late
    return torch.tensor(longform.stitch_numpy(x.numpy(), geo), dtype=torch.float32)
