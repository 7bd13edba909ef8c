"""The long-form mode end to end on the HIP engine (audio_style_transfer_amd/longform.py) -- run
on an MI355X.  Generated wavs (weights.synthetic_clips), synthetic weights, T = 4096, stack 0,
content layer 9, three windows, two epochs.  The runs are shared by the tests below."""
import glob
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from audio_style_transfer_amd import longform, summary, utils
from audio_style_transfer_amd.weights import synthetic_clips

pytestmark = pytest.mark.gpu

SR, T = 16000, 4096


def _run(tmp, tag, extra):
    argv = ['cont', 'style', '--batch_size', str(T), '--stack', '0', '--cont_lyrs', '9',
            '--epochs', '2', '--no_plots', '--dir', os.path.join(tmp, 'src'),
            '--outdir', os.path.join(tmp, 'out_' + tag), '--logdir', os.path.join(tmp, 'log_' + tag)]
    return longform.run(longform.make_parser().parse_args(argv + extra), log=lambda m: None)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    tmp = str(tmp_path_factory.mktemp('longform'))
    os.makedirs(os.path.join(tmp, 'src'))
    for name, seed in (('cont', 1000), ('style', 5000)):
        a = synthetic_clips(1, 2 * SR, seed)[0]
        wavfile.write(os.path.join(tmp, 'src', name + '.wav'), SR, (a * 32767).astype(np.int16))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)         # the synthetic-weights notice
        return {'w3': _run(tmp, 'w3', ['--windows', '3', '--seam', '0']),
                'w1': _run(tmp, 'w1', ['--windows', '1', '--seam', '0']),
                'seam': _run(tmp, 'seam', ['--windows', '3', '--seam', '50'])}


def _seam_mismatch(res):
    """Mean squared difference of the neighbours' audio over the fade spans."""
    g, x = res['geo'], res['x']
    d = []
    for k in range(g.n - 1):
        out_k = utils.inv_mu_law_numpy(x[k])[g.T - g.late - g.fade:g.T - g.late].astype(np.float64)
        in_k1 = utils.inv_mu_law_numpy(x[k + 1])[g.late:g.late + g.fade].astype(np.float64)
        d.append((out_k - in_k1) ** 2)
    return float(np.mean(d))


def test_output_files(runs):
    res = runs['w3']
    g = res['geo']
    assert res['epochs'] == 2 and g.n == 3
    sr, ep1 = wavfile.read(os.path.join(res['savepath'], 'ep-1.wav'))
    assert sr == SR and ep1.shape == (2 * g.hop + T - 2 * g.late,)
    assert np.isfinite(ep1.astype(np.float64)).all() and np.isfinite(res['x']).all()
    assert float(np.max(ep1)) > 0
    assert wavfile.read(os.path.join(res['savepath'], 'ori.wav'))[1].shape == ep1.shape
    assert wavfile.read(os.path.join(res['savepath'], 'style.wav'))[1].shape == (T - 2 * g.late,)
    ev = glob.glob(os.path.join(res['logdir'], '*tfevents*'))
    assert len(ev) == 1                                      # one event file for all windows
    rows = [e for e in summary.read_events(ev[0]) if e['scalars']]
    assert len(rows) >= 2 and all(np.isfinite(list(e['scalars'].values())).all() for e in rows)
    # the wav is the device stitch of the end points, peak-normalised
    a = longform.stitch_numpy(res['x'], g)
    np.testing.assert_allclose(res['audio'], a, rtol=0, atol=1e-6)


def test_window_0_is_the_one_window_run(runs):
    assert np.array_equal(runs['w3']['x'][0], runs['w1']['x'][0])


def test_seam_term_pulls_neighbours_together(runs):
    """A direction check, not a quality claim: after epoch 1 the neighbours differ less over
    the fade spans with --seam 50 than with --seam 0."""
    off, on = _seam_mismatch(runs['w3']), _seam_mismatch(runs['seam'])
    print('seam mismatch after epoch 1 (mean squared difference over the fade spans): '
          '--seam 0: %.6g   --seam 50: %.6g' % (off, on))
    assert runs['seam']['epochs'] == 2
    assert on < off
