"""bench.py's plain run and --dump-outputs: the plain result line carries the headline
figure and nothing that takes a run of its own (those sit behind --full), --steps sets
the timed steps, and the dumped frame is the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("roofline", "plugin_cadence", "cpu_baseline", "parity", "postpass")


@pytest.fixture(scope="module")
def bench():
    os.environ.setdefault("WORLD_SIZE", "1")
    import bench as B
    return B


def test_full_and_dump_outputs_are_off_by_default(bench):
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_the_whole_small_frame(bench, tmp_path):
    rng = np.random.default_rng(1)
    img = torch.from_numpy(rng.standard_normal((48, 40, 4)).astype(np.float16))
    bench.dump_outputs(str(tmp_path / "new" / "dir"), img)
    got = np.load(tmp_path / "new" / "dir" / "frame.npy")
    assert got.dtype == np.float32 and got.shape == (48, 40, 4)
    assert np.array_equal(got, img.numpy().astype(np.float32))


def test_dump_outputs_samples_a_large_frame_the_same_way_every_time(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_FULL_BYTES", 1 << 12)       # 256 pixels of 16 B
    img = torch.arange(64 * 64 * 4, dtype=torch.float32).reshape(64, 64, 4)
    bench.dump_outputs(str(tmp_path / "a"), img)
    bench.dump_outputs(str(tmp_path / "b"), img)
    a, b = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "b" / "frame.npy")
    assert a.dtype == np.float32 and a.shape == (256, 4) and a.nbytes == 1 << 12
    assert np.array_equal(a, b)
    # whole pixels of the frame, each once, in frame order
    px = (a[:, 0] / 4).astype(np.int64)
    assert np.array_equal(a, img.reshape(-1, 4).numpy()[px])
    assert np.all(np.diff(px) > 0)


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_frame(tmp_path):
    """A plain run at a small size: the result line has the headline fields and none of
    the --full blocks, --steps is the number of timed steps, and frame.npy is the RGBA16F
    frame of the workload as float32 (the renderer's own render of the same view)."""
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    args = ["--gpus", "1", "--steps", "6", "--warmup", "2", "--size", "64", "--res", "128",
            "--dump-outputs", str(tmp_path)]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       capture_output=True, text=True, timeout=120, env=e, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 6 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    # value = samples per frame / time per frame
    assert d["value"] == pytest.approx(d["config"]["samples_per_frame"] / d["ms_per_step"] / 1e3,
                                       rel=2e-2)
    assert not [k for k in FULL_ONLY if k in d]
    assert sorted(os.listdir(tmp_path)) == ["frame.npy"]
    got = np.load(tmp_path / "frame.npy")
    assert got.dtype == np.float32 and got.shape == (128, 128, 4)

    from cpp_volume_rendering_amd import _native as N
    from cpp_volume_rendering_amd import datasets as D
    from cpp_volume_rendering_amd.renderer import (Camera, DataManager, RayCasting1Pass,
                                                   RenderingParameters, build_tf_rgbt, make_frame)
    dm = DataManager()
    dm.SetVolume(D.marschner_lobb_u8(64), D.voxel_scale(64))
    dm.SetTransferFunction(build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA),
                           build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA, extinction_input=True))
    r = RayCasting1Pass(0)
    r.SetExternalResources(dm, RenderingParameters(128, 128, light_position=D.LIGHT_LIST0_POSITION))
    assert r.Init(128, 128)
    cam = Camera(**D.INITIAL_STATE_CAMERA)
    r.PrepareRender(cam)
    img = torch.zeros((128, 128, 4), dtype=torch.float16, device="cuda:0")
    r.device.set_stream(torch.cuda.current_stream().cuda_stream)
    r.render_to(make_frame(cam, 128, 128), N.Output(img.data_ptr(), None, None, 1, N.FORMAT_RGBA16F))
    torch.cuda.synchronize()
    want = img.float().cpu().numpy()
    r.Clean()
    assert (want[..., 3] > 0).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
