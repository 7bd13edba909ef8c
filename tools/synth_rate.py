#!/usr/bin/env python3
"""Device time per sample step of the WaveNet decoder at the default network.

  python tools/synth_rate.py [--batches 1,16,256] [--steps 2048] [--warmup 256] [--repeats 3]
  python tools/synth_rate.py --kernel-stats DIR [--batches 1]

For each batch size: a Decoder with seeded synthetic weights, ``--warmup`` steps, then HIP events
around ``--steps`` steps replayed from the 16-step graph, ``--repeats`` times (the median and the
spread are reported).  Prints one JSON line per batch size with the measured time and the two
floors it can be set against: the step's weight bytes over 6 TB/s (weights are fp32, read once
per 16-clip tile) and the graph's kernel count times 1.2 / 1.5 us per dependent kernel boundary.

--kernel-stats DIR runs itself once under ``rocprofv3 --kernel-trace --stats`` (a run of its own,
in a child process) and prints the decoder kernels' rows of the statistics.
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


def measure(batch, steps, warmup, repeats, W):
    import numpy as np
    import torch
    from audio_style_transfer_amd import synthesis
    K = 16
    total = warmup + steps * repeats + K
    R = -(-total // synthesis.HOP)
    rng = np.random.RandomState(0)
    dec = synthesis.Decoder(batch, W, graph_steps=K)
    try:
        dec.start(rng.randn(batch, R, 16), rng.rand(batch, total))
        dec.run(warmup)
        times = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps // K):
                dec.graph.replay()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / (steps // K * K))     # us per step
        assert dec.position() == warmup + (steps // K * K) * repeats
    finally:
        dec.close()
    times.sort()
    n_w = sum(int(v.size) for k, v in W.items() if k.endswith('/W'))
    kernels = 2 * 30 + 2
    tiles = -(-batch // 16)
    return dict(batch=batch, us_per_step=times[len(times) // 2], us_min=times[0], us_max=times[-1],
                steps=steps // K * K, repeats=repeats, weight_mb=n_w * 4 / 1e6,
                floor_weights_us=n_w * 4 / 6e12 * 1e6, floor_weights_per_tile_us=tiles * n_w * 4 / 6e12 * 1e6,
                kernels_per_step=kernels, floor_launch_us=[kernels * 1.2, kernels * 1.5],
                samples_per_s_per_clip=1e6 / times[len(times) // 2])


def kernel_stats(out_dir, batches):
    os.makedirs(out_dir, exist_ok=True)
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-T', '--output-format', 'csv', '-d', out_dir, '-o', 'run',
           '--', sys.executable, os.path.abspath(__file__), '--batches', batches, '--steps', '512',
           '--warmup', '64', '--repeats', '1']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    sys.stdout.write(r.stdout[-2000:])
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        return r.returncode
    for path in glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True):
        rows = [row for row in csv.DictReader(open(path)) if 'k_dec_' in row.get('Name', '')]
        for row in rows:
            print(json.dumps({k: row[k] for k in ('Name', 'Calls', 'TotalDurationNs', 'AverageNs', 'Percentage')
                              if k in row}))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--batches', default='1,16,256')
    ap.add_argument('--steps', type=int, default=2048)
    ap.add_argument('--warmup', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--kernel-stats', default=None, metavar='DIR')
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, args.batches)
    import torch
    if not torch.cuda.is_available():
        sys.exit('synth_rate needs a GPU: a time measured elsewhere says nothing')
    from audio_style_transfer_amd.weights import synthetic_decoder_weights
    W = synthetic_decoder_weights(0)
    for b in [int(v) for v in args.batches.split(',')]:
        print(json.dumps(measure(b, args.steps, args.warmup, args.repeats, W)), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
