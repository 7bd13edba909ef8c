"""The NSynth encoding on libastyle.so: a drop-in for fastgen.encode (nsynth/wavenet/
fastgen.py:86-113) and the embeddings CLI (nsynth/wavenet/nsynth_save_embeddings.py).

The encoding is the encoder's 16-channel bottleneck averaged over 512-sample hops
(model.py:121-128), [T / 512, 16] per clip: 30 block kernels, then k_encpool_fwd
(ast_encoding).

  python -m audio_style_transfer_amd.encoding --source_path DIR --save_path DIR
         [--checkpoint_path P] [--sample_length 64000] [--batch_size 16]

takes the sorted *.wav files of --source_path in batches of --batch_size (the last batch filled
by repeating its last file) and writes one <name>_embeddings.npy per real file into --save_path
(created if missing).  <name> is formed as the reference forms it
(nsynth_save_embeddings.py:113): ``.strip(".wav")`` strips *characters*, not a suffix, so
flute.wav -> flute but wave.wav -> e (and two files may collide); kept, so the output names are
the reference's.  A file shorter than --sample_length fails with a message (the reference fails
there too, inside np.array on the ragged batch).
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import warnings

import numpy as np

from . import utils

HOP = 512      # ae_hop_length (model.py:24)


def trim_for_encoding(wav_data, sample_length, hop_length=HOP):
    """nsynth/utils.py:139-167: at most ``sample_length`` samples and no more than the data
    holds (2-D: every row has the first row's length), rounded down to a whole number of hops;
    returns (the data cut to that length along its last axis, the length)."""
    wav_data = np.asarray(wav_data)
    if wav_data.ndim not in (1, 2):
        raise ValueError('wav_data must be 1-D or 2-D, got %d-D' % wav_data.ndim)
    n = min(int(sample_length), wav_data.shape[-1])
    n -= n % hop_length
    return wav_data[..., :n], n


def embedding_name(wavfile):
    """nsynth_save_embeddings.py:113: the file's base name with the *characters* '.', 'w', 'a',
    'v' stripped from both ends (not the suffix): flute.wav -> flute, wave.wav -> e."""
    return '%s_embeddings.npy' % wavfile.split('/')[-1].strip('.wav')


def batches(wavfiles, batch_size):
    """nsynth_save_embeddings.py:90-98: (files of the batch, filled to batch_size by repeating
    its last file; number of real files) per batch."""
    for start in range(0, len(wavfiles), batch_size):
        real = list(wavfiles[start:start + batch_size])
        yield real + (batch_size - len(real)) * [real[-1]], len(real)


def _weights(checkpoint_path, weights):
    if weights is not None:
        return weights
    from .methods import load_weights
    from .weights import synthetic_weights
    w = load_weights(checkpoint_path) if checkpoint_path else None
    if w is None:
        warnings.warn('no checkpoint at %r (neither <prefix>.index nor an .npz); '
                      'using seeded synthetic encoder weights' % (checkpoint_path,))
        w = synthetic_weights(0)
    return w


def encode(wav_data, checkpoint_path=None, sample_length=64000, weights=None, precision='split',
           engine_cls=None, device=None):
    """fastgen.encode (fastgen.py:86-113): wav_data [sample_length] or [mb, sample_length] audio
    in [-1, 1] -> the encoding, numpy float32 [mb, R, 16], R = trimmed length / 512 ([1, R, 16]
    for 1-D input).  ``weights`` (TF-named arrays) overrides ``checkpoint_path`` (a checkpoint-V2
    prefix or an .npz); ``engine_cls`` / ``device``: tests substitute a CPU stand-in."""
    import torch
    wav_data = np.asarray(wav_data)
    if wav_data.ndim == 1:
        wav_data = wav_data[None]
    wav_data, T = trim_for_encoding(wav_data, sample_length)
    if T < HOP:
        raise ValueError('encode needs at least %d samples, got %d' % (HOP, wav_data.shape[-1]))
    if engine_cls is None:
        from .engine import StyleEngine as engine_cls
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    # the taps only size the loss workspace, which encode never uses: the smallest set
    eng = engine_cls(wav_data.shape[0], T, [0], [0], precision=precision, device=device,
                     weights=_weights(checkpoint_path, weights), encoding=True)
    try:
        x = torch.tensor(utils.mu_law_numpy(wav_data), dtype=torch.float32, device=device)
        return eng.encoding(x).cpu().numpy()
    finally:
        if hasattr(eng, 'close'):
            eng.close()


def load_clip(path, sample_length, sr=16000):
    """nsynth/utils.py:50-67: the file at ``sr``, its first ``sample_length`` samples."""
    audio, _ = utils.load_audio(path, sr=sr)
    if len(audio) < sample_length:
        raise ValueError('%s has %d samples at %d Hz, fewer than --sample_length %d'
                         % (path, len(audio), sr, sample_length))
    return audio[:sample_length]


def save_embeddings(source_path, save_path, checkpoint_path=None, sample_length=64000,
                    batch_size=16, log=print, **kw):
    """nsynth_save_embeddings.py:70-118; returns the paths written.  ``kw`` goes to encode."""
    os.makedirs(save_path, exist_ok=True)
    wavfiles = sorted(os.path.join(source_path, f) for f in os.listdir(source_path)
                      if f.lower().endswith('.wav'))
    kw['weights'] = _weights(checkpoint_path, kw.get('weights'))
    written = []
    for k, (files, n_real) in enumerate(batches(wavfiles, batch_size)):
        log('On file number %d (batch %d).' % (k * batch_size, k + 1))
        wav = np.array([load_clip(f, sample_length) for f in files])
        enc = encode(wav, checkpoint_path, sample_length=sample_length, **kw)
        for f, e in zip(files[:n_real], enc):
            out = os.path.join(save_path, embedding_name(f))
            np.save(out, e)
            written.append(out)
    return written


def make_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--source_path', required=True, help='the directory of WAVs to yield embeddings from')
    p.add_argument('--save_path', required=True, help='the directory to save the embeddings')
    p.add_argument('--checkpoint_path', default=None,
                   help='TF checkpoint-V2 prefix or an .npz of TF-named encoder weights')
    p.add_argument('--sample_length', type=int, default=64000)
    p.add_argument('--batch_size', type=int, default=16)
    p.add_argument('--precision', default='split', choices=['fp32', 'split', 'bf16'])
    p.add_argument('--engine', default='audio_style_transfer_amd.engine:StyleEngine',
                   help='module:Class of the engine (tests substitute a CPU stand-in)')
    return p


def main(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    if args.sample_length < HOP or args.batch_size < 1:
        parser.error('--sample_length must be >= %d and --batch_size >= 1' % HOP)
    mod, cls = args.engine.split(':')
    m = importlib.import_module(mod)
    dev = getattr(m, 'DEVICE', None)
    try:
        save_embeddings(args.source_path, args.save_path, args.checkpoint_path, args.sample_length,
                        args.batch_size, precision=args.precision, engine_cls=getattr(m, cls),
                        device=dev)
    except ValueError as e:
        parser.error(str(e))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
