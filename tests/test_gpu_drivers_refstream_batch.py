"""test_ransac_softam -refstream T -batch F: the evaluation program's batched path (FrameBatch: the data set resident in HBM, F images per launch chain)
in the reference's own random stream (std::mt19937(seed + t) per OpenMP thread, core/thread_rand.cpp:40-69) -- FrameBatchOptions::refstream,
dsac_set_option("pi_refstream", 1).  It writes the same two result files as the per-image -refstream loop (dsac_sample_refstream + the replay path),
byte for byte, skipping the sub-sampler's draws on generator 0 by the same rule (-refsub)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dsac_amd", "host")
FILES = ("ransac_test_errors_obj_model_init.net_rdraw1_softam.txt", "ransac_test_loss_obj_model_init.net_rdraw1_softam.txt")


def run(d, args):
    d.mkdir()
    out = subprocess.run([os.path.join(HOST, "test_ransac_softam")] + [str(a) for a in args], cwd=str(d), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout, [open(os.path.join(str(d), f)).read() for f in FILES]


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("refsub", [1, 0])
def test_batched_refstream_evaluation_equals_the_per_image_loop(tmp_path, threads, refsub):
    base = ["-synth", 8, "-mw", 40, "-mh", 40, "-rI", 128, "-refstream", threads, "-refsub", refsub]
    so_b, files_b = run(tmp_path / "b4", base + ["-batch", 4])
    so_0, files_0 = run(tmp_path / "b0", base + ["-batch", 0])
    assert "reference random streams (threads): %d" % threads in so_b
    assert "batches of 4" in so_b and "one image per call" in so_0  # the path that was meant really ran
    assert files_b == files_0
    err = np.loadtxt(str(tmp_path / "b4" / FILES[0])).reshape(-1, 10)
    assert err.shape[0] == 8 and np.isfinite(err).all()
    # another thread count, or the counter stream, draws other sets
    _, files_c = run(tmp_path / "ctr", ["-synth", 8, "-mw", 40, "-mh", 40, "-rI", 128, "-batch", 4])
    assert files_c != files_b


def test_batched_refstream_passes_and_deferral_modes_agree(tmp_path):
    """Every pass re-initialises the generators (FrameBatch::processAll), so three passes enqueued back to back write what one pass writes, in every
    -defer mode."""
    base = ["-synth", 8, "-mw", 40, "-mh", 40, "-rI", 128, "-refstream", 1, "-batch", 4]
    _, ref = run(tmp_path / "p1", base)
    for tag, extra in (("d0", ["-defer", 0, "-passes", 3]), ("d1", ["-defer", 1, "-passes", 3]), ("d2", ["-defer", 2, "-passes", 3])):
        _, got = run(tmp_path / tag, base + extra)
        assert got == ref, tag
