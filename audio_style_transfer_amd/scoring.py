"""Scoring under the NSynth autoencoder on libastyle.so: the probability the WaveNet decoder
assigns to a waveform given an encoding, as the mean negative log-likelihood per sample that
Config.build returns as ``loss`` (nsynth/wavenet/model.py:213-214, 264, 310-320).

The waveform is quantised to 256 mu-law bins, the decoder runs teacher-forced over the whole clip
(ast_dec_score, synthesis.Decoder.score) with the training graph's input (bin - 128) / 128, and
the score is -mean_t log softmax(logits[t])[bin[t]] in nats, also in bits per sample (/ ln 2).
Conditioned on the clip's own encoding it is the reconstruction loss; conditioned on another
clip's encoding (--encodings) it says how well the waveform still fits that clip's content as the
model sees it.

  python -m audio_style_transfer_amd.scoring --source_path DIR_OR_FILE --save_path DIR
         [--checkpoint_path P] [--sample_length N] [--batch_size 1] [--gpu_number 0]
         [--encodings DIR] [--logp]

takes the sorted *.wav files of --source_path (the file selection of the synthesis CLI) and writes
scores.json, {name: {samples, nll_nats, bits_per_sample}}, into --save_path; with --logp also
<name>_logp.npy, the log-likelihood per sample.  Each file is cut to at most --sample_length
samples and a whole number of 512-sample hops, as encoding.encode cuts it.  --encodings DIR
conditions each file on DIR/<name>_embeddings.npy (the name rule of the embeddings CLI) instead of
its own encoding: this is how a style-transfer output is scored against its content clip.

One deviation from the reference: a sample of exactly 1.0 quantises to bin 256 there, which it
cannot score; here the bin is clamped to 0..255.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from . import encoding, synthesis, utils

HOP = synthesis.HOP


def quantize(wav):
    """floor(mu_law(wav)) + 128 as model.py:213 (utils.mu_law in float32, as the graph computes
    it), clamped to 0..255; int32, the shape of ``wav``."""
    x = np.asarray(wav, dtype=np.float32)
    mu = np.float32(255)
    out = np.sign(x) * np.log(np.float32(1) + mu * np.abs(x)) / np.float32(np.log(256.0))
    return np.clip(np.floor(out * np.float32(128)).astype(np.int32) + 128, 0, 255)


def score(wav_data, checkpoint_path=None, sample_length=64000, encodings=None, weights=None,
          engine_cls=None, encode_fn=None, device=None):
    """wav_data [n] or [B, n] audio in [-1, 1], cut as encoding.encode cuts it (at most
    ``sample_length``, a whole number of hops) -> dict(nll [B] nats per sample, bits [B] =
    nll / ln 2, logp [B, T]).  Conditioned on ``encodings`` [B, R, 16] with R = T / 512 when
    given, else on encoding.encode of the same audio.  ``weights`` (TF-named decoder arrays)
    overrides ``checkpoint_path``; ``engine_cls`` / ``encode_fn`` / ``device``: tests substitute
    CPU stand-ins."""
    wav = np.asarray(wav_data)
    if wav.ndim == 1:
        wav = wav[None]
    wav, T = encoding.trim_for_encoding(wav, sample_length)
    if T < HOP:
        raise ValueError('score needs at least %d samples, got %d' % (HOP, wav.shape[-1]))
    if encodings is None:
        enc = (encode_fn or encoding.encode)(wav, checkpoint_path, sample_length=sample_length)
    else:
        enc = encodings
    enc = np.asarray(enc, dtype=np.float32)
    if enc.ndim == 2:
        enc = enc[None]
    if enc.shape != (wav.shape[0], T // HOP, synthesis.N_Z):
        raise ValueError('encodings %s do not fit %d clips of %d samples: expected %s'
                         % (enc.shape, wav.shape[0], T, (wav.shape[0], T // HOP, synthesis.N_Z)))
    if engine_cls is None:
        engine_cls = synthesis.Decoder
    eng = engine_cls(1, synthesis._decoder_weights(checkpoint_path, weights), device=device)
    try:
        r = eng.score(quantize(wav), enc, input_mode=1)
    finally:
        eng.close()
    return dict(nll=r['nll'], bits=r['bits'], logp=r['logp'])


def score_name(wavfile):
    """The key of a file in scores.json: its base name without the extension."""
    return os.path.splitext(os.path.basename(wavfile))[0]


def make_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--source_path', default='', help='a .wav file or a directory of .wav files')
    p.add_argument('--save_path', default='', help='output directory (scores.json)')
    p.add_argument('--checkpoint_path', default='model.ckpt-200000',
                   help='TF checkpoint-V2 prefix (or an .npz of TF-named weights)')
    p.add_argument('--sample_length', type=int, default=64000, help='at most this many samples per file')
    p.add_argument('--batch_size', type=int, default=1, help='files scored per call')
    p.add_argument('--gpu_number', type=int, default=0, help='the GPU to use')
    p.add_argument('--encodings', default=None, metavar='DIR',
                   help='condition each file on DIR/<name>_embeddings.npy instead of its own encoding')
    p.add_argument('--logp', action='store_true', help='also write <name>_logp.npy per file')
    return p


def _load_encoding(enc_dir, wavfile, T):
    path = os.path.join(enc_dir, encoding.embedding_name(wavfile))
    if not os.path.isfile(path):
        raise ValueError('%s: no encoding %s' % (wavfile, path))
    e = np.load(path)
    if e.ndim == 3 and e.shape[0] == 1:
        e = e[0]
    if e.ndim != 2 or e.shape[1] != synthesis.N_Z or e.shape[0] != T // HOP:
        raise ValueError('%s: %s holds an encoding %s, but the %d samples scored need [%d, %d]'
                         % (wavfile, path, e.shape, T, T // HOP, synthesis.N_Z))
    return e


def score_files(args, score_fn=None):
    """The CLI's body; returns the dictionary written to scores.json.  Files of one batch are cut
    to the shortest of them (then to whole hops)."""
    source_path = synthesis._shell_path(args.source_path)
    save_path = synthesis._shell_path(args.save_path)
    if not save_path:
        raise RuntimeError('Must specify a save_path.')
    if score_fn is None:
        score_fn = score
    files, postfix = synthesis.select_files(source_path)      # sorted; a folder's .wav files win
    if postfix != '.wav':
        raise RuntimeError('scoring takes .wav files, %s holds none' % source_path)
    os.makedirs(save_path, exist_ok=True)
    scores = {}
    for start in range(0, len(files), args.batch_size):
        batch_files = files[start:start + args.batch_size]
        clips = [utils.load_audio(f, sr=16000)[0][:args.sample_length] for f in batch_files]
        wav, T = encoding.trim_for_encoding(np.stack([c[:min(len(c) for c in clips)] for c in clips]),
                                            args.sample_length)
        if T < HOP:
            raise ValueError('%s: fewer than %d samples' % (', '.join(batch_files), HOP))
        enc = None
        if args.encodings:
            enc = np.stack([_load_encoding(synthesis._shell_path(args.encodings), f, T) for f in batch_files])
        r = score_fn(wav, args.checkpoint_path, sample_length=args.sample_length, encodings=enc)
        for k, f in enumerate(batch_files):
            name = score_name(f)
            scores[name] = dict(samples=int(T), nll_nats=float(r['nll'][k]), bits_per_sample=float(r['bits'][k]))
            if args.logp:
                np.save(os.path.join(save_path, name + '_logp.npy'), r['logp'][k])
    with open(os.path.join(save_path, 'scores.json'), 'w') as f:
        json.dump(scores, f, indent=1, sort_keys=True)
    return scores


def main(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    if args.batch_size < 1 or args.sample_length < HOP:
        parser.error('--batch_size must be >= 1 and --sample_length >= %d' % HOP)
    import torch
    torch.cuda.set_device(args.gpu_number)
    try:
        score_files(args)
    except ValueError as e:
        parser.error(str(e))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
