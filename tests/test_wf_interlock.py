"""The shade interlock of the wavefront executor (csrc/wf_plan.h: wf_shade_wait): its decisions on the CPU, and on the GPU that
gating the shade launches changes when kernels run and nothing of what they compute.

The GPU tests use S-cornell at 128 x 128: every job of that film is a small job to the default plan (its sub-pipelines share the trace grid, each
item has a slot of its own: exempt from the interlock), so each case runs twice -- as it is, where no launch may wait, and with
MCPT_WF_SMALL_JOB_SPLIT=0 and pools of 65 536 slots, where the same jobs run on the full grid with more items than slots and are gated.
MCPT_WF_DEBUG makes the library print the number of waits of every call; the tests read it."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.kit import ROOT

SIZE, DEPTH, SEED = 128, 8, 11
MODES = {"small-job": {}, "full-grid": {"MCPT_WF_SMALL_JOB_SPLIT": "0", "MCPT_WF_POOL_SLOTS": "65536"}}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_interlock_decisions_form_one_chain_and_never_wait_on_nothing(tmp_path):
    """tests/wf_interlock_check.cpp replays the executor's loop on the CPU: rounds of 2 and 3 sub-pipelines that finish and leave the full grid at
    arbitrary rounds, known-length, small-job and single-lane calls, probes, deterministic mode."""
    exe = str(tmp_path / "wf_interlock_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "wf_interlock_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) >= 1000000


@pytest.fixture(scope="module")
def scene(pkg):
    return pkg.scenes.cornell_box(SIZE, SIZE)


def _renderer(pkg, scene, monkeypatch, interlock, mode, depth=DEPTH, lanes=None):
    """A context made under the given knobs (the library reads them when a context is made)."""
    for name in ("MCPT_WF_SMALL_JOB_SPLIT", "MCPT_WF_POOL_SLOTS", "MCPT_WF_LANES"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MCPT_WF_INTERLOCK", "1" if interlock else "0")
    monkeypatch.setenv("MCPT_WF_DEBUG", "1")
    for name, value in MODES[mode].items():
        monkeypatch.setenv(name, value)
    if lanes:
        monkeypatch.setenv("MCPT_WF_LANES", str(lanes))
    return pkg.Renderer(scene, max_depth=depth)


def _waits(capfd):
    """The waits of every render call since the last look at the library's stderr."""
    return [int(n) for n in re.findall(r"\[wf\] interlock waits=(\d+)", capfd.readouterr().err)]


def _film(r):
    r.sync()
    film = r.read_accum()
    assert film.shape == (SIZE, SIZE, 4) and np.all(np.isfinite(film))
    return film


SPP = 32                                                    # of the same-film test


@pytest.fixture(scope="module")
def samples(pkg, scene):
    """Every sample of the same-film test on its own: (sum of the samples, sum of their magnitudes, all of them non-negative) per channel, in
    fp64.  Sample i is the film of a one-sample call with first_sample = i (counter-based random numbers: the same value it has inside the
    32-sample call); such a call splits the tiles over the sub-pipelines and stores without atomics, so the film holds the sample itself."""
    with pytest.MonkeyPatch.context() as mp:
        for name in ("MCPT_WF_SMALL_JOB_SPLIT", "MCPT_WF_POOL_SLOTS", "MCPT_WF_LANES", "MCPT_WF_DEBUG"):
            mp.delenv(name, raising=False)
        mp.setenv("MCPT_WF_INTERLOCK", "0")
        r = pkg.Renderer(scene, max_depth=DEPTH)
    total = np.zeros((SIZE, SIZE, 3)); magnitude = np.zeros((SIZE, SIZE, 3)); nonneg = np.ones((SIZE, SIZE, 3), bool)
    for i in range(SPP):
        r.clear(); r.render(1, seed=SEED, first_sample=i)
        f = _film(r)
        assert np.all(f[..., 3] == 1.0)
        x = f[..., :3].astype(np.float64)
        total += x; magnitude += np.abs(x); nonneg &= x >= 0
    r.close()
    return total, magnitude, nonneg


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_same_film_with_and_without_the_interlock(pkg, scene, samples, monkeypatch, capfd, mode):
    """32 spp on two sub-pipelines, with the interlock and without.  The samples are the same (counter-based random numbers); what differs is the
    order in which the film's fp32 atomics add them, as it does from run to run.  An fp32 sum of n terms x_i in any order is within
    (n - 1) 2^-24 (1 + O(n 2^-24)) sum |x_i| of the exact sum, so two orders differ by less than n 2^-23 sum |x_i|.

    Asserted per channel: where every sample is non-negative, sum |x_i| is the sum itself and the two films agree within spp 2^-23 relative.
    Few channels are like that: samples can be negative, only 3 355 of this film's 49 152 channels hold no negative sample and 171 sums
    are negative themselves -- and where samples cancel a reordering moves the sum by more than that fraction of it (two renders without the
    interlock have differed by 1.1e-05 of a channel that held 0.0003).  There the same factor is applied to what the error really scales with, sum |x_i|, taken from the samples rendered one by
    one (the `samples` fixture).  Both films are also held to the exact sum of those samples within half that bound each."""
    total, magnitude, nonneg = samples
    films = {}
    for interlock in (False, True):
        r = _renderer(pkg, scene, monkeypatch, interlock, mode)
        capfd.readouterr()
        r.render(SPP, seed=SEED)
        films[interlock] = _film(r)
        waits = _waits(capfd)
        r.close()
        assert len(waits) == 1
        if interlock and mode == "full-grid":
            assert waits[0] >= 8, waits                                   # at least one wait per iteration of a depth-8 job
        else:
            assert waits[0] == 0, waits
        assert np.all(films[interlock][..., 3] == float(SPP))
    a, b = films[True][..., :3].astype(np.float64), films[False][..., :3].astype(np.float64)
    bound = SPP * 2.0 ** -23
    err = np.abs(a - b)
    print("channels with non-negative samples only: %d of %d; largest difference there %.3g of the channel, elsewhere %.3g of sum |x_i| (bound %.3g)" % (
        int(nonneg.sum()), nonneg.size, float(np.max(err[nonneg] / np.maximum(b[nonneg], 1e-30))),
        float(np.max(err[~nonneg] / magnitude[~nonneg])) if (~nonneg).any() else 0.0, bound))
    assert nonneg.any() and b.max() > 0
    assert np.all(err[nonneg] <= bound * b[nonneg])                       # the issue's bound, where its premise holds
    assert np.all(err[~nonneg] <= bound * magnitude[~nonneg])             # the same factor of what the error scales with, where samples cancel
    for film in (a, b):                                                   # and each film is the sum of these very samples
        assert np.all(np.abs(film - total) <= 0.5 * bound * magnitude)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("spp,depth", [(3, DEPTH), (33, 0)])
def test_uneven_lanes_return_with_an_exact_count_plane(pkg, scene, monkeypatch, capfd, mode, spp, depth):
    """3 spp: sub-pipeline 0 has one sample per pixel, a known-length job enqueued whole, beside a polled one -- nobody waits.  33 spp at depth 0
    (no depth limit: no known length): 16 and 17 samples, both polled, one finishes first and the survivor goes on alone."""
    r = _renderer(pkg, scene, monkeypatch, True, mode, depth=depth)
    capfd.readouterr()
    r.render(spp, seed=SEED)
    film = _film(r)
    waits = _waits(capfd)
    r.close()
    assert np.all(film[..., 3] == float(spp))
    assert len(waits) == 1
    if spp == 33 and mode == "full-grid":
        assert waits[0] >= 4, waits
    else:
        assert waits[0] == 0, waits


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_three_sub_pipelines(pkg, scene, monkeypatch, capfd, mode):
    spp = 32
    r = _renderer(pkg, scene, monkeypatch, True, mode, lanes=3)
    capfd.readouterr()
    r.render(spp, seed=SEED)
    film = _film(r)
    waits = _waits(capfd)
    r.close()
    assert np.all(film[..., 3] == float(spp))
    assert len(waits) == 1 and (waits[0] >= 12 if mode == "full-grid" else waits[0] == 0), waits


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_two_calls_back_to_back_reuse_the_events(pkg, scene, monkeypatch, capfd, mode):
    """No sync between the calls: the second call's launches are enqueued, and its events re-recorded, while the first is still running."""
    r = _renderer(pkg, scene, monkeypatch, True, mode)
    capfd.readouterr()
    r.render(16, seed=SEED, first_sample=0)
    r.render(16, seed=SEED, first_sample=16)
    film = _film(r)
    waits = _waits(capfd)
    r.close()
    assert np.all(film[..., 3] == 32.0)
    assert len(waits) == 2 and all(w >= 8 if mode == "full-grid" else w == 0 for w in waits), waits


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_one_render_tiles_call(pkg, scene, monkeypatch, capfd, mode):
    """Every other 8 x 8 tile of the film: those pixels hold 32 samples, the others none."""
    spp = 32
    r = _renderer(pkg, scene, monkeypatch, True, mode)
    capfd.readouterr()
    r.render_tiles(spp, SEED, 0, 2, 1)
    film = _film(r)
    waits = _waits(capfd)
    r.close()
    ys, xs = np.mgrid[0:SIZE, 0:SIZE]
    owned = ((ys // 8) * (SIZE // 8) + xs // 8) % 2 == 1
    assert np.all(film[..., 3][owned] == float(spp)) and np.all(film[~owned] == 0)
    assert len(waits) == 1 and (waits[0] >= 8 if mode == "full-grid" else waits[0] == 0), waits
