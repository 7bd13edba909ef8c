"""Long-form mode of the CLI: one content file, many overlapping windows, one stitched output.

The reference optimises one --batch_size clip taken at --start (methods.py:183-216).  Here
consecutive windows of the content file are laid onto the engine's batch dimension, each window
is optimised by the reference's protocol (methods.py:164-181, as batch.run_rank runs it), and the
windows are joined on the device (ast_stitch) into one signal:

  python -m audio_style_transfer_amd.longform cont_fn style_fn [methods.py flags]
         [--windows N | --seconds S] [--fade F] [--seam MU] [--chunk C] [--engine module:Class]

Geometry (geometry()): T = --batch_size, late = the guard the reference drops at both ends of a
clip (methods.py:39), F = --fade, hop = T - 2 late - F.  Window k starts at st + k hop with
st = int(start sr - late) (methods.py:192), so window 0 is the clip the reference CLI optimises;
neighbours overlap by F valid samples and are crossfaded with sin^2 weights that sum to 1.
Per window: phi_c is the window's own content embedding, the style target is
l2norm(phi(window) + phi_t - phi_s) (methods.py:194-203), every epoch a fresh L-BFGS-B
minimize(maxiter 100) from fp32(x) on the device (engine.LbfgsLoop), stopped for a window once an
epoch used fewer than 50 evaluations; the split range guard reruns a flagged window's epoch on
fp32 kernels.  After every epoch ep-N.wav is the stitched signal of all windows divided by its
maximum; ori.wav is the content file over the same span, style.wav as the reference writes it;
the event file holds every evaluation's loss scalars summed over the windows.

--seam MU > 0 adds the seam anchor term (ast_set_anchor) from epoch 1 on: each window is pulled,
on its fade-in and fade-out spans, towards the previous epoch's stitched signal, i.e. both
neighbours towards the same blend.  Within an epoch the loss stays a fixed function of each
window's own x.  Whether the term improves what a listener hears is unmeasured: it is off by
default (MU = 0: the windows are fully independent problems).

More windows than --chunk C run as consecutive chunks of C within every epoch; with --seam > 0 a
later chunk's first window is anchored on its fade-in span to the audio the earlier chunk's last
window reached in that epoch (epoch 0 included).  The stitch runs once over all windows.

Out of scope, refused: more than one GPU (the seam term across ranks would need an exchange),
--optimizer scipy, --resume.
"""
from __future__ import annotations

import collections
import importlib
import os
import sys
import time
import warnings

import numpy as np

from . import methods, summary, utils

Geometry = collections.namedtuple('Geometry', 'T late fade hop n n_out')


def late_of(T):
    """methods.py:39: the guard dropped at both ends of a T-sample clip."""
    return (T - (T // 4096) * 4000) // 2


def geometry(T, fade, n=1):
    """The long-form geometry of n windows of T samples crossfaded over `fade` samples: the one
    place the kernel's arguments, the anchor weights and the tests take their numbers from.
    Output sample s is file position st + late + s; n_out = (n - 1) hop + T - 2 late."""
    T, fade, n = int(T), int(fade), int(n)
    if T < 4096:
        raise ValueError('--batch_size %d < 4096: no sample survives the guard (2 late = T)' % T)
    late = late_of(T)
    if fade < 0:
        raise ValueError('--fade must be >= 0 (got %d)' % fade)
    if 2 * fade > T - 2 * late:
        raise ValueError('--fade %d: 2 fade > T - 2 late = %d, a window\'s fade-in and fade-out '
                         'would meet' % (fade, T - 2 * late))
    if n < 1:
        raise ValueError('need at least one window (got %d)' % n)
    hop = T - 2 * late - fade
    return Geometry(T, late, fade, hop, n, (n - 1) * hop + T - 2 * late)


def seam_spans(geo, k):
    """Local index spans [(lo, hi)] of window k shared with a neighbour: its fade-in (k > 0) and
    its fade-out (k < n - 1); none at the outer ends of the first and last window."""
    T, late, F = geo.T, geo.late, geo.fade
    out = []
    if F > 0 and k > 0:
        out.append((late, late + F))
    if F > 0 and k < geo.n - 1:
        out.append((T - late - F, T - late))
    return out


def window_weights(geo, k):
    """Crossfade weight [T] (float64) of window k: 0 in the guards, r((i - late + 1/2) / F) on the
    fade-in, r((T - late - i - 1/2) / F) on the fade-out, 1 elsewhere; r(u) = sin^2(pi u / 2).
    The fade-out is evaluated as its equal 1 - r(1 - u), one minus the neighbour's fade-in at the
    same sample (as the kernel blends), so that a pair's weights sum to 1 without a rounding."""
    T, late, F = geo.T, geo.late, geo.fade
    w = np.zeros(T)
    w[late:T - late] = 1.0
    r = lambda u: np.sin(0.5 * np.pi * u) ** 2
    for lo, hi in seam_spans(geo, k):
        i = np.arange(lo, hi, dtype=np.float64)
        w[lo:hi] = r((i - late + 0.5) / F) if lo == late else 1.0 - r((i - (T - late - F) + 0.5) / F)
    return w


def window_starts(geo, st):
    return [st + k * geo.hop for k in range(geo.n)]


def stitch_numpy(x, geo):
    """ast_stitch restated in numpy float64: x [n, T] mu-law units -> audio [n_out]."""
    x = np.asarray(x)
    assert x.shape == (geo.n, geo.T), (x.shape, geo)
    out = np.zeros(geo.n_out)
    V = geo.T - 2 * geo.late
    for k in range(geo.n):
        a = utils.inv_mu_law_numpy(x[k]).astype(np.float64)
        out[k * geo.hop:k * geo.hop + V] += (window_weights(geo, k) * a)[geo.late:geo.T - geo.late]
    return out


def count_windows(T, fade, n_samples, st, windows=None, seconds=None, sr=16000):
    """--windows N, else --seconds S (the smallest N whose output covers S seconds), else every
    whole window that fits in the content file; refuses windows past the file's end."""
    g = geometry(T, fade)
    fit = (n_samples - st - T) // g.hop + 1 if n_samples - st >= T else 0
    if windows is not None:
        n = int(windows)
    elif seconds is not None:
        need = int(np.ceil(float(seconds) * sr))
        n = max(1, -(-(need - (T - 2 * g.late)) // g.hop) + 1)
    else:
        n = fit
    if n < 1:
        raise ValueError('no whole window of %d samples fits in the content file from sample %d '
                         '(%d samples)' % (T, st, n_samples))
    if n > fit:
        raise ValueError('%d windows need %d samples from sample %d; the content file has %d'
                         % (n, (n - 1) * g.hop + T, st, n_samples))
    return n


EXTRA = methods.EXTRA_FLAGS + ('windows', 'seconds', 'fade', 'seam', 'chunk', 'engine')


def make_parser():
    p = methods.make_parser(description=__doc__.split('\n\n')[0])
    g = p.add_mutually_exclusive_group()
    g.add_argument('--windows', type=int, default=None, help='number of windows')
    g.add_argument('--seconds', type=float, default=None,
                   help='the smallest number of windows whose output covers this many seconds '
                        '(default: every whole window that fits in the content file)')
    p.add_argument('--fade', type=int, default=256,
                   help='crossfade between neighbouring windows in samples (default 256, about '
                        '16 ms at 16 kHz: a judgement call, nobody has measured it)')
    p.add_argument('--seam', type=float, default=0.0,
                   help='weight MU of the seam anchor term (default 0 = off, the windows are '
                        'independent; its effect on audio quality is unmeasured)')
    p.add_argument('--chunk', type=int, default=256, help='windows optimised together')
    p.add_argument('--engine', default='audio_style_transfer_amd.engine:StyleEngine',
                   help='module:Class of the engine; the module also provides LbfgsLoop and '
                        'stitch (tests substitute a CPU stand-in)')
    p.set_defaults(optimizer='device')
    return p


def out_dirs(args):
    """The run's output and log directories: methods.get_dir's naming, the long-form flags left
    out of the name as methods.EXTRA_FLAGS are."""
    kw = {k: v for k, v in vars(args).items() if k not in EXTRA}
    return (utils.gt_s_path(utils.crt_t_fol(args.outdir), **kw),
            utils.gt_s_path(utils.crt_t_fol(args.logdir), **kw))


def _engine_module(spec):
    mod, cls = spec.split(':')
    m = importlib.import_module(mod)
    return getattr(m, cls), getattr(m, 'LbfgsLoop'), getattr(m, 'stitch'), getattr(m, 'DEVICE', None)


def check_args(args):
    if args.optimizer != 'device':
        raise ValueError('the long-form mode runs the device L-BFGS-B; --optimizer scipy is out of scope')
    if args.resume:
        raise ValueError('--resume is out of scope for long-form runs')
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise ValueError('the long-form mode runs on one GPU (the seam term across ranks would '
                         'need an exchange)')
    if args.seam < 0 or not np.isfinite(args.seam):
        raise ValueError('--seam must be finite and >= 0')
    if args.chunk < 1:
        raise ValueError('--chunk must be >= 1')
    if getattr(args, 'enc', 0.0) != 0:
        raise ValueError('--enc (the encoding term) is out of scope for long-form runs; use methods')


def run(args, log=print):
    """The long-form run; returns {'x': end points [n, T] float64, 'audio': the last stitched
    signal (float64, not normalised), 'geo': Geometry, 'savepath', 'logdir', 'epochs': run}."""
    import torch
    check_args(args)
    Eng, Loop, stitch_fn, devname = _engine_module(args.engine)
    dev = torch.device(devname) if devname else torch.device('cuda', torch.cuda.current_device())
    T, sr, F, mu = args.batch_size, args.sr, args.fade, float(args.seam)
    geometry(T, F)                                                   # refuse before any work
    cont, style = (methods.get_fpath(f, args) for f in (args.cont_fn, args.style_fn))
    aud, _ = utils.load_audio(cont, sr=sr, audio_channel=0)
    late = late_of(T)
    st = int(args.start * sr - late)                                 # methods.py:192
    if st < 0:
        raise ValueError('--start %g lies within the first window\'s guard' % args.start)
    geo = geometry(T, F, count_windows(T, F, len(aud), st, args.windows, args.seconds, sr))
    n, hop, V = geo.n, geo.hop, T - 2 * late
    savepath, logdir = out_dirs(args)
    figdir = os.path.join(savepath, 'fig')
    os.makedirs(figdir, exist_ok=True)
    weights = methods.load_weights(args.weights) if args.weights else None
    # a one-clip GatysNet for the file-level style embeddings (methods.py:97-111, 186-187)
    net = methods.GatysNet(savepath, args.ckpt_path, logdir, figdir, args.stack, T, sr,
                           args.cont_lyrs, args.channels, args.cnt_channels, args.gatys,
                           args.style_lyrs, precision=args.precision, device=dev, weights=weights,
                           plots=not args.no_plots, optimizer='device', engine_cls=Eng)
    phi_t = net.get_style_phi(style)
    phi_s = net.get_style_phi(cont, show_mat=False)
    utils.write_wav(os.path.join(savepath, 'ori.wav'), aud[st + late:st + late + geo.n_out], sr)
    style_aud, _ = utils.load_audio(style, sr=sr, audio_channel=0)
    utils.write_wav(os.path.join(savepath, 'style.wav'), style_aud[st:st + T][late:-late], sr)
    xw = np.stack([utils.mu_law_numpy(aud[s:s + T]) for s in window_starts(geo, st)]).astype(np.float32)

    C = min(int(args.chunk), n)
    chunks = [(k0, min(k0 + C, n)) for k0 in range(0, n, C)]
    ref = torch.zeros(C, T, device=dev)          # the anchor's persistent buffers, filled in place
    w = torch.zeros(C, T, device=dev)
    tgt = {}                                     # the targets' persistent buffers
    engines, loops, anchored = {}, {}, {}

    def engine(precision):
        if precision not in engines:
            e = Eng(C, T, net.cont_lyr_ids, net.style_lyr_ids, cnt_channels=args.cnt_channels,
                    nb_channels=args.channels, gatys=args.gatys, lambd=args.lambd,
                    precision=precision, device=dev, weights=net.weights)
            e.set_gamma(args.gamma)
            engines[precision], loops[precision], anchored[precision] = e, Loop(e, maxiter=100), False
        return engines[precision]

    def set_targets(k0, k1):
        """phi_c / the style target of windows k0..k1 (padded to C with the last one) from one
        batched embeds call, into the persistent buffers."""
        idx = list(range(k0, k1)) + [k1 - 1] * (C - (k1 - k0))
        emb_c, emb_s = engine(args.precision).embeds(torch.tensor(xw[idx], device=dev))
        es = emb_s.cpu().numpy()
        phi = np.empty_like(es)
        for b in range(C):                                           # methods.py:199-203
            p = es[b] + phi_t - phi_s
            phi[b] = p / np.sqrt(np.maximum(np.sum(p * p, axis=(1, 2), keepdims=True), 1e-12))
        if not tgt:
            tgt['c'], tgt['s'] = emb_c.clone(), torch.tensor(phi, dtype=torch.float32, device=dev)
        else:
            tgt['c'].copy_(emb_c)
            tgt['s'].copy_(torch.tensor(phi, dtype=torch.float32, device=dev))

    def fill_anchor(ep, k0, k1, prev, x):
        """ref / w of windows k0..k1 in place; True when some weight is set."""
        w.zero_()
        on = False
        if mu <= 0 or F == 0:
            return False
        if prev is not None:             # the previous epoch's stitched signal at each window
            ref[:k1 - k0, late:T - late] = prev.unfold(0, V, hop)[k0:k1]
            for b, k in enumerate(range(k0, k1)):
                for lo, hi in seam_spans(geo, k):
                    w[b, lo:hi] = 1.0
                    on = True
        if k0 > 0:                       # a later chunk: the earlier chunk's audio of this epoch
            a = utils.inv_mu_law_numpy(x[k0 - 1])[T - late - F:T - late]
            ref[0, late:late + F] = torch.tensor(a, dtype=torch.float32, device=dev)
            w[0, late:late + F] = 1.0
            on = True
        return on

    def minimize(precision, sel, x0):
        lp = loops[precision]
        info = lp.minimize(torch.tensor(x0, dtype=torch.float64),
                           active=torch.tensor(sel.astype(np.int32)))
        _, xe = lp.state(with_x=True)
        return info, xe.cpu().numpy(), lp.history(info)

    from . import _lib
    guard = _lib.RANGE_NONFINITE | _lib.RANGE_ACT | _lib.RANGE_GRAD
    x = np.full((n, T), 1e-6).astype(np.float32).astype(np.float64)        # methods.py:49-54
    i_ = np.zeros(n, int)
    active = np.ones(n, bool)
    prec = [args.precision] * n
    writer = summary.EventWriter(logdir)
    prev, audio, step0, done = None, None, 0, 0
    since = time.time()
    for ep in range(args.epochs):
        if not active.any():
            break
        hist = [None] * n
        for k0, k1 in chunks:
            nb = k1 - k0
            run_c = np.zeros(C, bool)
            run_c[:nb] = active[k0:k1]
            if not run_c.any():
                continue
            if ep == 0 or len(chunks) > 1:
                set_targets(k0, k1)
            on = fill_anchor(ep, k0, k1, prev, x)
            pad = list(range(k0, k1)) + [k1 - 1] * (C - nb)
            x0 = x[pad].astype(np.float32).astype(np.float64)        # each epoch from fp32(x)
            pc = [prec[k] for k in pad]
            pending = {p: run_c & np.array([q == p for q in pc]) for p in ('split', 'bf16', 'fp32')}
            for p in ('split', 'bf16', 'fp32'):
                sel = pending[p]
                if not sel.any():
                    continue
                e = engine(p)
                e.set_targets(tgt['c'], tgt['s'])
                if on != anchored[p]:        # (set or cleared only when it changes: the buffers
                    e.set_anchor(ref, w, mu) if on else e.set_anchor(None)   # are filled in place)
                    anchored[p] = on
                info, xs, hs = minimize(p, sel, x0)
                if p == 'split':                                     # the range guard
                    f = e.range_flags().cpu().numpy()
                    bad = sel & ((f & guard) != 0)
                    if bad.any():
                        log('split precision: range flags on windows %s; their epoch reruns on '
                            'fp32 kernels' % [k0 + b for b in np.flatnonzero(bad)])
                        for b in np.flatnonzero(bad):
                            prec[k0 + b] = 'fp32'
                        pending['fp32'] = pending['fp32'] | bad
                        sel = sel & ~bad
                for b in np.flatnonzero(sel):
                    x[k0 + b], hist[k0 + b] = xs[b], hs[b]
                    i_[k0 + b] = int(info[b, 2])
                    if i_[k0 + b] < 50:                              # methods.py:180-181
                        active[k0 + b] = False
        tl = time.time() - since
        ran = [h for h in hist if h is not None]
        nmax = max(len(h) for h in ran)
        for k in range(nmax):                # every evaluation's scalars, summed over the windows
            pv = np.sum([h[k] for h in ran if len(h) > k], axis=0)
            writer.add_scalars({'loss/content_loss': pv[1], 'loss/style_loss': pv[2],
                                'loss/regularizer': pv[3], 'loss/main_loss': pv[0]}, step0 + k)
            if not k % 5:
                log('Ep %d/%d-it %d(%d)-tlapse %.4fs-%d windows-loss%.4f-%.4f-%.4f-%.4f' % (
                    ep + 1, args.epochs, k, step0, tl, len(ran), *pv))
        writer.flush()
        step0 = nmax                                                 # methods.py:147-157: i_ + i
        prev = stitch_fn(torch.tensor(x, dtype=torch.float32, device=dev), late, F)
        audio = prev.cpu().numpy().astype(np.float64)
        utils.write_wav(os.path.join(savepath, 'ep-{}.wav'.format(ep)), audio / np.max(audio), sr)
        done = ep + 1
    writer.close()
    for e in engines.values():
        e.close()
    return {'x': x, 'audio': audio, 'geo': geo, 'savepath': savepath, 'logdir': logdir,
            'epochs': done}


def main(argv=None):
    parser = make_parser()
    args = parser.parse_args(argv)
    try:
        check_args(args)
        geometry(args.batch_size, args.fade)
    except ValueError as e:
        parser.error(str(e))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)     # the synthetic-weights notice
        run(args)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
