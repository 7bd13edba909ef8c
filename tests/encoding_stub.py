"""CPU stand-in engine for the embeddings CLI's tests (tests/test_encoding.py), in the style of
longform_stub: ``--engine encoding_stub:EncStubEngine`` runs audio_style_transfer_amd.encoding
without a GPU.  Its "encoding" is a fixed linear map of the hop means of x, enc[b, r, j] =
(j + 1) * mean(x[b, hop r]), so a test can tell which clip a row came from.  Every construction
is appended to encoding_stub.BUILT as (batch, T, kwargs)."""
from __future__ import annotations

import torch

DEVICE = 'cpu'
BUILT = []


class EncStubEngine:

    def __init__(self, batch, T, cont_ids, style_ids, device=None, **kw):
        assert torch.device(device).type == 'cpu' and T % 512 == 0
        self.batch, self.T = int(batch), int(T)
        BUILT.append((self.batch, self.T, dict(kw)))

    def encoding(self, x):
        assert x.shape == (self.batch, self.T) and x.dtype == torch.float32
        m = x.reshape(self.batch, self.T // 512, 512).double().mean(2)
        return (m[:, :, None] * torch.arange(1, 17, dtype=torch.float64)).float()
