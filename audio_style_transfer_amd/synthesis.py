"""The NSynth WaveNet decoder on libastyle.so: a drop-in for fastgen.synthesize / load_batch
(nsynth/wavenet/fastgen.py:116-212) and the generation CLI (nsynth/wavenet/nsynth_generate.py).

An encoding [R, 16] (encoding.encode, or a *_embeddings.npy of the embeddings CLI) becomes
R * 512 samples of audio, one sample per step: ~2 n_layers + 2 kernels per step (ast_dec_step),
captured once into a HIP graph of ``graph_steps`` steps and replayed.

  python -m audio_style_transfer_amd.synthesis --source_path DIR_OR_FILE --save_path DIR
         [--npy_only] [--checkpoint_path P] [--sample_length N] [--batch_size 1] [--gpu_number 0]

takes the .wav files of --source_path (the .npy files when it holds no .wav, or with --npy_only),
sorted, in batches of --batch_size, and writes gen_<name>.wav per input into --save_path.  Wav
inputs go through encoding.encode first.

Two departures from the reference, both where it cannot run: load_batch stacks [R, 16] encodings to
[batch, R, 16] (np.vstack there yields [batch * R, 16], which fastgen.synthesize cannot index; a
file holding [1, R, 16] is taken as [R, 16]), and a single-file --source_path picks its kind from
the file's extension (the reference leaves ``postfix`` unset on that path).
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys
import warnings

import numpy as np

from . import _lib, utils
from .weights import decoder_weight_shapes

HOP = 512       # Config().ae_hop_length (model.py:154)
N_Z = 16
NBIN = 256
DEFAULTS = dict(width=512, skip_width=256, n_layers=30, n_stages=10, hop=HOP)   # model.py:45-50


class Decoder(object):
    """One decoder context (ast_dec_*): weights, then per synthesis ``start`` (upload, reset),
    ``run`` (graph replays) or ``step`` (one eager step), and the outputs."""

    def __init__(self, batch, weights=None, device=None, width=512, skip_width=256, n_layers=30,
                 n_stages=10, hop=HOP, graph_steps=16):
        import torch
        self.torch = torch
        self.lib = _lib.load()
        self.h = None
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        device = torch.device(device)
        if device.type != 'cuda':
            raise _lib.AstError('Decoder needs a GPU device, got %s' % device)
        self.device = device
        self.batch, self.hop, self.graph_steps = int(batch), int(hop), int(graph_steps)
        self.n_stages = int(n_stages)
        self.sizes = dict(width=width, skip_width=skip_width, n_layers=n_layers, n_z=N_Z)
        cfg = _lib.AstDecCfg(batch, width, skip_width, n_layers, n_stages, N_Z, hop)
        h = ctypes.c_void_p()
        _lib.check(self.lib.ast_dec_create(ctypes.byref(cfg), device.index or 0, ctypes.byref(h)))
        self.h = h
        self.graph = None
        self.total = 0
        self._pos = torch.zeros(1, dtype=torch.int32, device=device)
        if weights is not None:
            self.set_weights(weights)

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _p(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def close(self):
        if getattr(self, 'h', None):
            self.graph = None
            self._score_work = None
            self.torch.cuda.synchronize(self.device)
            self.lib.ast_dec_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def set_weight(self, name, value):
        a = np.ascontiguousarray(value, dtype=np.float32)
        _lib.check(self.lib.ast_dec_set_weight(self.h, name.encode(),
                                               a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a.size))

    def set_weights(self, weights):
        for name in decoder_weight_shapes(**self.sizes):
            if name not in weights:
                raise _lib.AstError('decoder weights: no variable %s' % name)
            self.set_weight(name, weights[name])

    def restore(self, prefix):
        _lib.check(self.lib.ast_dec_restore(self.h, str(prefix).encode()))

    # ------------------------------------------------------------------ one synthesis
    def start(self, enc, u, force=None, want_pmf=False, out=None):
        """enc [B, R, 16]; u [B, total] uniforms, total <= R hop; force None or int [B, total]
        (teacher forcing).  ``out``: caller-owned device tensors bins (int32), audio (float32)
        [B, total] and optionally pmf [B, total, 256] to write into.  Resets the queues."""
        torch = self.torch
        dev = self.device
        self.enc = torch.as_tensor(np.asarray(enc, dtype=np.float32), device=dev).contiguous()
        self.u = torch.as_tensor(np.asarray(u, dtype=np.float32), device=dev).contiguous()
        B, self.R, nz = self.enc.shape
        self.total = int(self.u.shape[1])
        if B != self.batch or nz != N_Z or self.u.shape[0] != B:
            raise _lib.AstError('start: enc %s / u %s do not fit batch %d'
                                % (tuple(self.enc.shape), tuple(self.u.shape), self.batch))
        self.force = None
        if force is not None:
            f = np.asarray(force)
            if f.shape != (B, self.total) or f.min() < 0 or f.max() >= NBIN:
                raise _lib.AstError('start: force must be [batch, total] bins in 0..255')
            self.force = torch.as_tensor(f.astype(np.int32), device=dev).contiguous()
        out = out or {}
        self.bins_dev = out.get('bins')
        self.audio_dev = out.get('audio')
        self.pmf_dev = out.get('pmf')
        if self.bins_dev is None:
            self.bins_dev = torch.zeros(B, self.total, dtype=torch.int32, device=dev)
        if self.audio_dev is None:
            self.audio_dev = torch.zeros(B, self.total, dtype=torch.float32, device=dev)
        if self.pmf_dev is None and want_pmf:
            self.pmf_dev = torch.zeros(B, self.total, NBIN, dtype=torch.float32, device=dev)
        self.graph = None
        # one eager step before any capture (every kernel has run once), then init_ops again:
        # the reset makes the run start from the same state either way
        self.reset()
        self.step()
        self.reset()

    def reset(self):
        _lib.check(self.lib.ast_dec_reset(self.h, self._stream()))

    def step(self):
        """One eager sample step (a no-op at the end)."""
        _lib.check(self.lib.ast_dec_step(self.h, self._p(self.enc), self.R, self._p(self.u),
                                         self._p(self.force), self.total, self._p(self.bins_dev),
                                         self._p(self.audio_dev), self._p(self.pmf_dev), self._stream()))

    def run(self, n_steps=None):
        """At least ``n_steps`` more steps (default: to the end) as replays of the captured graph
        of ``graph_steps`` steps; steps past the end do nothing.  Returns the position."""
        torch = self.torch
        if n_steps is None:
            n_steps = self.total
        if self.graph is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):      # capture records the steps without running them
                for _ in range(self.graph_steps):
                    self.step()
            self.graph = g
        for _ in range(-(-int(n_steps) // self.graph_steps)):
            self.graph.replay()
        return self.position()

    def position(self):
        _lib.check(self.lib.ast_dec_position(self.h, self._p(self._pos), self._stream()))
        return int(self._pos.item())

    # ------------------------------------------------------------------ scoring
    def score(self, bins, enc, input_mode=0, want_pmf=False, want_logits=False):
        """The decoder teacher-forced on ``bins`` int [B, T] (0..255) under ``enc`` [B, R, 16],
        T <= R hop (ast_dec_score): dict of logp [B, T] = log p(bins[t] | bins[<t], enc),
        nll [B] (nats per sample), bits = nll / ln 2 and optionally pmf / logits [B, T, 256], as
        numpy arrays.  input_mode 0 feeds the synthesis table back, 1 (bin - 128) / 128 (the
        training graph).  B is independent of the context's batch; the synthesis state is not
        touched.  The work area is a cached tensor that grows as needed."""
        torch = self.torch
        dev = self.device
        b = np.asarray(bins)
        e = np.asarray(enc, dtype=np.float32)
        if b.ndim != 2 or b.shape[0] < 1 or b.shape[1] < 1 or not np.issubdtype(b.dtype, np.integer):
            raise _lib.AstError('score: bins must be integers [batch, T], got %s %s' % (b.dtype, b.shape))
        if e.ndim != 3 or e.shape[0] != b.shape[0] or e.shape[2] != N_Z:
            raise _lib.AstError('score: enc %s does not fit bins %s' % (e.shape, b.shape))
        if b.min() < 0 or b.max() >= NBIN:
            raise _lib.AstError('score: bins must lie in 0..255, got %d..%d' % (b.min(), b.max()))
        B, T = b.shape
        R = e.shape[1]
        if T > R * self.hop:
            raise _lib.AstError('score: T %d exceeds R hop = %d' % (T, R * self.hop))
        if input_mode not in (0, 1):
            raise _lib.AstError('score: input_mode %r, must be 0 or 1' % (input_mode,))
        st = self._score_buffers(B, T, want_pmf, want_logits)
        st['bins'].copy_(torch.as_tensor(b.astype(np.int32)))
        enc_dev = torch.as_tensor(e, device=dev).contiguous()
        self._score_launch(st, enc_dev, R, input_mode)
        out = dict(logp=st['logp'].cpu().numpy(), nll=st['nll'].cpu().numpy())
        out['bits'] = out['nll'] / np.float32(np.log(2.0))
        for k in ('pmf', 'logits'):
            if st[k] is not None:
                out[k] = st[k].cpu().numpy()
        return out

    def _score_buffers(self, B, T, want_pmf=False, want_logits=False):
        torch = self.torch
        dev = self.device
        n = ctypes.c_size_t()
        c = self.sizes
        cfg = _lib.AstDecCfg(self.batch, c['width'], c['skip_width'], c['n_layers'], self.n_stages, N_Z, self.hop)
        _lib.check(self.lib.ast_dec_score_workspace_bytes(ctypes.byref(cfg), B, T, ctypes.byref(n)))
        work = getattr(self, '_score_work', None)
        if work is None or work.numel() < n.value:
            self._score_work = work = None          # release before growing
            self._score_work = work = torch.empty(n.value, dtype=torch.uint8, device=dev)
        return dict(work=work, need=n.value, B=B, T=T,
                    bins=torch.empty(B, T, dtype=torch.int32, device=dev),
                    logp=torch.empty(B, T, dtype=torch.float32, device=dev),
                    nll=torch.empty(B, dtype=torch.float32, device=dev),
                    pmf=torch.empty(B, T, NBIN, dtype=torch.float32, device=dev) if want_pmf else None,
                    logits=torch.empty(B, T, NBIN, dtype=torch.float32, device=dev) if want_logits else None)

    def _score_launch(self, st, enc_dev, R, input_mode):
        """Launches only (graph-capturable): ast_dec_score on the buffers of _score_buffers."""
        _lib.check(self.lib.ast_dec_score(self.h, self._p(st['bins']), self._p(enc_dev), st['B'], R, st['T'],
                                          int(input_mode), self._p(st['work']), st['work'].numel(),
                                          self._p(st['logp']), self._p(st['nll']), self._p(st['pmf']),
                                          self._p(st['logits']), self._stream()))

    def bins(self):
        return self.bins_dev.cpu().numpy()

    def audio(self):
        return self.audio_dev.cpu().numpy()

    def pmf(self):
        return self.pmf_dev.cpu().numpy()


def dec_tables():
    """The library's bin -> audio and bin -> next-input tables (ast_dec_tables; host only)."""
    a = np.empty(NBIN, dtype=np.float32)
    x = np.empty(NBIN, dtype=np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    _lib.check(_lib.load().ast_dec_tables(a.ctypes.data_as(fp), x.ctypes.data_as(fp)))
    return a, x


def draw_uniforms(total, batch, seed=None):
    """The reference's draws (fastgen.py:46): np.random.rand(batch) once per step, in step order,
    from the global generator, or from RandomState(seed).  [batch, total] float64."""
    rng = np.random if seed is None else np.random.RandomState(seed)
    return np.ascontiguousarray(rng.rand(total, batch).T)


def _decoder_weights(checkpoint_path, weights):
    if weights is not None:
        return weights
    from . import checkpoint
    from .weights import synthetic_decoder_weights
    if checkpoint.is_checkpoint(checkpoint_path):
        return checkpoint.decoder_weights(checkpoint_path)
    if checkpoint_path and str(checkpoint_path).endswith('.npz') and os.path.isfile(checkpoint_path):
        return dict(np.load(checkpoint_path))
    warnings.warn('no checkpoint at %r (neither <prefix>.index nor an .npz); '
                  'using seeded synthetic decoder weights' % (checkpoint_path,))
    return synthetic_decoder_weights(0)


def save_batch(batch_audio, batch_save_paths):
    """fastgen.py:154-157."""
    for audio, name in zip(batch_audio, batch_save_paths):
        utils.write_wav(name, audio, 16000)


def synthesize(encodings, save_paths, checkpoint_path=None, samples_per_save=1000, weights=None,
               seed=None, engine_cls=None, device=None):
    """fastgen.synthesize (fastgen.py:160-212): encodings [batch, R, 16] -> audio [batch, R * 512]
    float32, written to ``save_paths`` every ``samples_per_save`` samples and at the end.
    ``weights`` (TF-named arrays) overrides ``checkpoint_path``; ``seed``: draw the uniforms from
    RandomState(seed) instead of the global generator; ``engine_cls`` / ``device``: tests
    substitute a CPU stand-in for Decoder."""
    enc = np.asarray(encodings, dtype=np.float32)
    if enc.ndim != 3 or enc.shape[2] != N_Z or enc.shape[1] < 1:
        raise ValueError('encodings must be [batch, time, %d], got %s' % (N_Z, enc.shape))
    save_paths = list(save_paths)
    batch, R = enc.shape[0], enc.shape[1]
    if len(save_paths) != batch:
        raise ValueError('%d save paths for %d encodings' % (len(save_paths), batch))
    if samples_per_save < 1:
        raise ValueError('samples_per_save must be >= 1')
    total = R * HOP
    u = draw_uniforms(total, batch, seed)
    if engine_cls is None:
        engine_cls = Decoder
    eng = engine_cls(batch, _decoder_weights(checkpoint_path, weights), device=device)
    try:
        eng.start(enc, u)
        pos = 0
        while pos < total:
            pos = eng.run(samples_per_save)
            print('Sample: {}'.format(pos), end='\r', flush=True)
            save_batch(eng.audio(), save_paths)
        audio = eng.audio()
        save_batch(audio, save_paths)
        return audio
    finally:
        eng.close()


def load_batch(files, sample_length=64000):
    """fastgen.load_batch (fastgen.py:116-151): .wav (at 16 kHz, at most sample_length samples) or
    .npy files, chosen by the first file's extension, zero-padded to the longest; audio
    [batch, length] or encodings [batch, length, dims]."""
    is_npy = os.path.splitext(files[0])[1] == '.npy'
    data = []
    for f in files:
        if is_npy:
            d = np.load(f)
            if d.ndim == 3 and d.shape[0] == 1:
                d = d[0]
        else:
            d = utils.load_audio(f, sr=16000)[0][:sample_length]
        data.append(d)
    n = max(d.shape[0] for d in data)
    out = np.zeros((len(data), n) + data[0].shape[1:], dtype=np.float64 if is_npy else data[0].dtype)
    for i, d in enumerate(data):
        out[i, :d.shape[0]] = d
    return out


def select_files(source_path, npy_only=False):
    """nsynth_generate.py:51-71: (sorted files, postfix).  A directory: its .wav files, the .npy
    files when it has no .wav or with npy_only; a .wav / .npy file: itself; else nothing."""
    if os.path.isdir(source_path):
        names = os.listdir(source_path)
        exts = [os.path.splitext(f)[1] for f in names]
        if '.wav' in exts:
            postfix = '.wav'
        elif '.npy' in exts:
            postfix = '.npy'
        else:
            raise RuntimeError('Folder must contain .wav or .npy files.')
        postfix = '.npy' if npy_only else postfix
        return sorted(os.path.join(source_path, f) for f in names if f.lower().endswith(postfix)), postfix
    if source_path.lower().endswith(('.wav', '.npy')):
        return [source_path], source_path.lower()[-4:]
    return [], '.wav'


def save_names(files, save_path):
    """nsynth_generate.py:80-84."""
    return [os.path.join(save_path, 'gen_' + os.path.splitext(os.path.basename(f))[0] + '.wav')
            for f in files]


def _flag_bool(v):
    if v.lower() in ('true', 't', '1', 'yes'):
        return True
    if v.lower() in ('false', 'f', '0', 'no'):
        return False
    raise argparse.ArgumentTypeError('not a boolean: %r' % v)


def make_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--source_path', default='',
                   help='directory with either .wav files or precomputed encodings in .npy files; '
                        'wav files are used when present, else .npy files')
    p.add_argument('--npy_only', nargs='?', const=True, default=False, type=_flag_bool,
                   help='use only .npy files')
    p.add_argument('--save_path', default='', help='output directory')
    p.add_argument('--checkpoint_path', default='model.ckpt-200000',
                   help='TF checkpoint-V2 prefix (or an .npz of TF-named weights)')
    p.add_argument('--sample_length', type=int, default=100000000, help='max output file size in samples')
    p.add_argument('--batch_size', type=int, default=1, help='number of samples per batch')
    p.add_argument('--log', default='INFO', help='accepted for the reference command line; unused')
    p.add_argument('--gpu_number', type=int, default=0, help='the GPU to use')
    return p


def _shell_path(p):
    return os.path.abspath(os.path.expanduser(os.path.expandvars(p))) if p else p


def generate(args, synthesize_fn=None, encode_fn=None):
    """nsynth_generate.main (nsynth_generate.py:42-94); returns the files written."""
    source_path = _shell_path(args.source_path)
    save_path = _shell_path(args.save_path)
    if not save_path:
        raise RuntimeError('Must specify a save_path.')
    if synthesize_fn is None:
        synthesize_fn = synthesize
    if encode_fn is None:
        from .encoding import encode as encode_fn
    files, postfix = select_files(source_path, args.npy_only)
    os.makedirs(save_path, exist_ok=True)
    written = []
    for start in range(0, len(files), args.batch_size):
        batch_files = files[start:start + args.batch_size]
        names = save_names(batch_files, save_path)
        data = load_batch(batch_files, sample_length=args.sample_length)
        enc = data if postfix == '.npy' else encode_fn(data, args.checkpoint_path,
                                                       sample_length=args.sample_length)
        synthesize_fn(enc, names, checkpoint_path=args.checkpoint_path)
        written += names
    return written


def main(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    if args.batch_size < 1:
        parser.error('--batch_size must be >= 1')
    import torch
    torch.cuda.set_device(args.gpu_number)
    generate(args)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
