#!/usr/bin/env python3
"""Device time of decoder scoring (ast_dec_score) at the default network.

  python tools/score_rate.py [--batches 1,16] [--T 16384] [--warmup 2] [--repeats 5] [--steps 2048]
  python tools/score_rate.py --kernel-stats DIR [--batches 1]

For each batch size: a Decoder with seeded synthetic weights and random bins; ``--warmup`` scores,
then HIP events around each of ``--repeats`` scores (launches only: the inputs are on the device).
Prints one JSON line per batch size: the median ms per call and per clip, the achieved TFLOP/s
(2 flop per multiply-add of every product but the 3-tap startconv) against the 157.3 TF fp32 MFMA
roof and the time that roof allows, and the ratio to the step path teacher-forced on the same bins
in the same run (``--steps`` steps replayed from the 16-step graph at the same batch, scaled to T).

--kernel-stats DIR runs itself once under ``rocprofv3 --kernel-trace --stats`` (a run of its own,
in a child process) and prints the score kernels' rows of the statistics.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF_TF = 157.3


def measure(batch, T, warmup, repeats, steps, W):
    import numpy as np
    import torch
    from audio_style_transfer_amd import synthesis
    K = 16
    R = -(-T // synthesis.HOP)
    rng = np.random.RandomState(0)
    enc = rng.randn(batch, R, 16).astype(np.float32)
    bins = rng.randint(0, 256, size=(batch, T))
    macs = sum(int(v.size) for k, v in W.items() if k.endswith('/W') and not k.startswith('startconv'))
    dec = synthesis.Decoder(batch, W, graph_steps=K)
    try:
        st = dec._score_buffers(batch, T)
        st['bins'].copy_(torch.as_tensor(bins.astype(np.int32)))
        enc_dev = torch.as_tensor(enc, device=dec.device)
        for _ in range(warmup):
            dec._score_launch(st, enc_dev, R, 0)
        times = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dec._score_launch(st, enc_dev, R, 0)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))                               # ms per call
        times.sort()
        ms = times[len(times) // 2]
        nll = st['nll'].cpu().numpy()
        out = dict(batch=batch, T=T, ms_per_call=ms, ms_per_clip=ms / batch, ms_min=times[0], ms_max=times[-1],
                   repeats=repeats, macs_per_sample=macs, tflops=2.0 * macs * T * batch / (ms * 1e-3) / 1e12,
                   roof_tflops=ROOF_TF, floor_ms_per_clip=2.0 * macs * T / (ROOF_TF * 1e12) * 1e3,
                   work_mib=st['need'] / 2.0 ** 20, nll_first=float(nll[0]))
        out['roof_fraction'] = out['tflops'] / ROOF_TF
        if steps:
            n = min(steps // K * K, T // K * K)
            dec.start(enc, np.full((batch, T), 0.5, np.float32), force=bins)
            dec.run(K)                                                     # captures the graph
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n // K):
                dec.graph.replay()
            b.record()
            b.synchronize()
            us = a.elapsed_time(b) * 1e3 / n
            out.update(step_us=us, step_steps=n, step_ms_per_T=us * T * 1e-3, speedup_over_step=us * T * 1e-3 / ms)
        return out
    finally:
        dec.close()


def kernel_stats(out_dir, batches, T):
    os.makedirs(out_dir, exist_ok=True)
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-T', '--output-format', 'csv', '-d', out_dir, '-o', 'run',
           '--', sys.executable, os.path.abspath(__file__), '--batches', batches, '--T', str(T), '--warmup', '1',
           '--repeats', '3', '--steps', '0']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    sys.stdout.write(r.stdout[-2000:])
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        return r.returncode
    for path in glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True):
        rows = [row for row in csv.DictReader(open(path)) if 'k_score_' in row.get('Name', '')]
        for row in rows:
            print(json.dumps({k: row[k] for k in ('Name', 'Calls', 'TotalDurationNs', 'AverageNs', 'Percentage')
                              if k in row}))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--batches', default='1,16')
    ap.add_argument('--T', type=int, default=16384)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=2048, help='steps of the step path timed for the ratio; 0: skip')
    ap.add_argument('--kernel-stats', default=None, metavar='DIR')
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, args.batches, args.T)
    import torch
    if not torch.cuda.is_available():
        sys.exit('score_rate needs a GPU: a time measured elsewhere says nothing')
    from audio_style_transfer_amd.weights import synthetic_decoder_weights
    W = synthetic_decoder_weights(0)
    for b in [int(v) for v in args.batches.split(',')]:
        print(json.dumps(measure(b, args.T, args.warmup, args.repeats, args.steps, W)), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
