"""bench.py's multi-GPU orchestration on CPU: ``python bench.py --gpus 2`` with no
launcher starts its own two rank processes (spawn_ranks: fresh interpreters,
torch.distributed.run's environment), which deal the frame's bands, gather them
into rank 0's frame (BandGather over gloo, the mirror of vx_mgpu_gather), take the
max time over ranks and print one JSON line.  --standin swaps the HIP band
renderer for a CPU stand-in; everything else is the path the 8-GPU run takes."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, timeout=240):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_spawns_its_own_ranks_gloo(built):
    j = _bench("--gpus", "2", "--standin", "--full", "--steps", "4", "--warmup", "1", "--inflight", "2")
    assert j["n_gpus"] == 2 and j["steps"] == 4 and j["warmup"] == 1
    assert j["scaling"] == "strong"                       # N > 1 defaults to C4 (7680x4320 for every N)
    assert j["config"]["workload"].startswith("C4")
    assert j["config"]["standin_frame_ok"] is True        # every band arrived in rank 0's frame
    sh = j["config"]["shards"]
    assert sh["assignment"].startswith("round-robin") and "gloo" in sh["gather"]
    assert j["value"] > 0 and j["ms_per_step"] > 0
    assert j["config"]["primary_rays"] == j["config"]["width"] * j["config"]["height"]


def test_bench_eight_ranks_standin_c4(built):
    """the driver's 8-GPU run rehearsed on CPU -- bench.py
    --gpus 8 spawns eight ranks, deals C4's 4320 rows (narrowed frames in the
    stand-in) in the band height vx_mgpu_band_rows picks, gathers over gloo and
    emits one line carrying the render / gather split and the deal's balance."""
    j = _bench("--gpus", "8", "--standin", "--full", "--steps", "3", "--warmup", "1", "--inflight", "2", timeout=600)
    assert j["n_gpus"] == 8 and j["steps"] == 3
    assert j["config"]["workload"].startswith("C4") and j["config"]["height"] == 4320
    assert j["config"]["standin_frame_ok"] is True
    sh = j["config"]["shards"]
    assert sh["unit"].startswith("32-row")                # vx_mgpu_band_rows(4320, 8)
    assert sh["rows_per_rank_max_over_mean"] <= 1.01
    sp = sh["split_ms"]
    assert sp["render_ms"] > 0 and sp["gather_ms"] > 0, sp
    assert sp["gather_bytes"] == j["config"]["width"] * 4 * (4320 - 544)   # all rows but rank 0's 544


def test_plain_run_times_one_block_and_dumps_the_last_frame(built, tmp_path):
    """Without --full: exactly --steps timed frames in one block, none of --full's
    extra legs, and --dump-outputs writes rank 0's gathered frame of the last step
    (float32, every band's stand-in value, the sampled rows named)."""
    import numpy as np
    from voxmap_amd.dist import band_rows_for, band_rows_of
    j = _bench("--gpus", "2", "--standin", "--steps", "3", "--warmup", "1", "--inflight", "2",
               "--dump-outputs", str(tmp_path / "out"))
    assert j["full"] is False and j["steps"] == 3 and j["ms_per_step"] > 0 and j["value"] > 0
    t = j["config"]["timing"]
    assert t["blocks"] == 1 and t["steps_per_block"] == 3
    assert j["config"]["shards"]["split_ms"] is None and "cpu_baseline" not in j
    frame = np.load(tmp_path / "out" / "frame.npy")
    rows = np.load(tmp_path / "out" / "frame_rows.npy").astype(int)
    H, W = j["config"]["height"], j["config"]["width"]
    assert frame.dtype == np.float32 and frame.shape == (len(rows), W, 4) and frame.nbytes <= 64 << 20
    assert len(set(rows.tolist())) == len(rows) and rows.min() >= 0 and rows.max() < H
    band = band_rows_for(H, 2)
    want = np.empty(H, np.float32)
    j_last = (1 + 3 - 1) % 2                               # warmup + steps frames over 2 frames in flight
    for b in range(-(-H // band)):
        want[band_rows_of(b, H, band)] = (b * 7 + j_last) % 251
    assert np.array_equal(frame, np.broadcast_to(want[rows, None, None], frame.shape))


def test_dump_row_sample_is_fixed_and_bounded():
    """A frame too large to dump whole (C3: 3840x2160 RGBA as float32 = 133 MB)
    keeps a sorted, seeded row sample: the same rows every run, within 64 MB."""
    import importlib.util

    import numpy as np
    spec = importlib.util.spec_from_file_location("voxmap_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a, b = bench.dump_rows(2160, 3840), bench.dump_rows(2160, 3840)
    assert np.array_equal(a, b) and np.array_equal(a, np.unique(a)) and 0 <= a[0] and a[-1] < 2160
    assert 256 <= len(a) < 2160 and len(a) * 3840 * 16 <= 64 << 20
    assert np.array_equal(bench.dump_rows(72, 128), np.arange(72))
