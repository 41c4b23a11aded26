"""tools/style_transfer_amd.py --scale_image: the blur + resize + crop of the reference's video examples on the GPU path
(`--scale_on gpu`, vtoonify_amd/scale.py through the video driver's `prescale`), from `--landmarks` alone -- neither cv2 nor
dlib is importable in these runs.  Host emulation; one rank and a 2-rank gloo world.  The frames that come out must equal
those of the same command on clips pre-cropped by the restatement of tests/test_frame_scale.py, run without --scale_image.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from test_frame_scale import ref_axis, ref_crop
from test_style_transfer_cli import _emu, _free_port

sys.path.insert(0, os.path.join(REPO, "tools"))
import style_transfer_amd as cli  # noqa: E402

# eyes 100 apart -> scale 0.64, centre (80,40)*0.64 = (51.2,25.6); 64x88 -> round(40.96) x round(56.32) = 41 x 56;
# padding (12,12,8,8): left 39//8*8 = 32, right min(63,56)//8*8 = 56, top 18//8*8 = 16, bottom min(34,41)//8*8 = 32; one pass
HS, WS, PADDING = 64, 88, (12, 12, 8, 8)
SCALED, LEFT, RIGHT, TOP, BOTTOM, PASSES = (41, 56), 32, 56, 16, 32, 1


def _clip(tmp_path, n=5, seed=7):
    g = np.random.default_rng(seed)
    frames = g.integers(0, 256, (n, HS, WS, 3), dtype=np.uint8)
    lm = np.zeros((68, 2))
    lm[36:42], lm[42:48] = (30, 40), (130, 40)
    xtab, ytab = ref_axis(LEFT, RIGHT, SCALED[1], WS, True), ref_axis(TOP, BOTTOM, SCALED[0], HS, False)
    crops = np.stack([ref_crop(f, PASSES, xtab, ytab) for f in frames], 0)
    maps = (g.standard_normal((n, 19, BOTTOM - TOP, RIGHT - LEFT)) * 4).astype(np.float32)
    for d, clip in (("src", frames), ("pre", crops)):
        os.makedirs(tmp_path / d)
        np.save(tmp_path / d / "clip.npy", clip)
    np.save(tmp_path / "lm.npy", lm)
    np.save(tmp_path / "maps.npy", maps)
    np.save(tmp_path / "code.npy", g.standard_normal((1, 18, 512)).astype(np.float32))
    return frames, crops


def _args(tmp_path, which, out, backbone="toonify", extra=()):
    scale = ["--scale_image", "--landmarks", str(tmp_path / "lm.npy"), "--padding", *map(str, PADDING)] if which == "src" else []
    return ["--content", str(tmp_path / which / "clip.npy"), "--video", "--parsing_map_path", str(tmp_path / "maps.npy"),
            "--intrinsic_code", str(tmp_path / "code.npy"), "--ckpt", "synthetic", "--backbone", backbone,
            "--output_path", str(out), "--batch_size", "2", "--depth", "2", "--precision", "bf16", *scale, *extra]


def _no_cv2_no_dlib(monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)        # `import cv2` raises ImportError
    monkeypatch.setitem(sys.modules, "dlib", None)


def test_options_are_additions():
    opt = cli.parse(["--scale_image"])
    assert opt.landmarks is None and opt.scale_on == "gpu"
    assert cli.parse(["--scale_on", "host", "--landmarks", "a.npy"]).scale_on == "host"
    with pytest.raises(SystemExit):
        cli.parse(["--scale_on", "somewhere"])


def test_scale_image_one_process_equals_precropped_clip(tmp_path, monkeypatch):
    _emu()
    _no_cv2_no_dlib(monkeypatch)
    _clip(tmp_path)
    rep = cli.main(_args(tmp_path, "src", tmp_path / "o_src"), device="cpu")
    got = np.load(rep["output"])
    assert rep["frames"] == 5 and got.shape == (5, 4 * (BOTTOM - TOP), 4 * (RIGHT - LEFT), 3) and got.dtype == np.uint8
    want = np.load(cli.main(_args(tmp_path, "pre", tmp_path / "o_pre"), device="cpu")["output"])
    assert np.array_equal(got, want)
    # without landmarks and without dlib the option stops with a message that names the way out
    with pytest.raises(SystemExit, match="--landmarks"):
        cli.main([a for a in _args(tmp_path, "src", tmp_path / "o_x") if a not in ("--landmarks", str(tmp_path / "lm.npy"))],
                 device="cpu")
    # the reference's host path is still there, and still needs cv2
    with pytest.raises(SystemExit, match="cv2"):
        cli.main(_args(tmp_path, "src", tmp_path / "o_y", extra=("--scale_on", "host")), device="cpu")


_WORKER = """
import os, sys
sys.modules["cv2"] = None; sys.modules["dlib"] = None          # neither is importable in this run
sys.path.insert(0, os.environ["VT_REPO"]); sys.path.insert(0, os.path.join(os.environ["VT_REPO"], "tests"))
sys.path.insert(0, os.path.join(os.environ["VT_REPO"], "tools"))
from emu import build_emu
from vtoonify_amd import _lib
_lib.use_library(build_emu.build())
import style_transfer_amd as cli
rep = cli.main(sys.argv[1:], device="cpu", backend="gloo")
print("rank", rep["rank"], "shard", rep["shard"], "ok")
"""


def test_scale_image_two_ranks_equal_precropped_clip(tmp_path):
    _emu()
    _clip(tmp_path)
    want = np.load(cli.main(_args(tmp_path, "pre", tmp_path / "o_pre", backbone="dualstylegan"), device="cpu")["output"])
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), VT_REPO=REPO, OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, str(script)] + _args(tmp_path, "src", tmp_path / "o_two", backbone="dualstylegan"),
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=900)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o}"
    assert "shard (0, 3)" in outs[0] and "shard (3, 5)" in outs[1]
    two = np.load(tmp_path / "o_two" / "clip_vtoonify_d.npy")
    assert two.shape == want.shape == (5, 64, 96, 3) and np.array_equal(two, want)


def test_cpu_flag_crops_with_the_host_form(tmp_path, monkeypatch):
    """--cpu --parsing_map_path: ScaleCrop.host feeds the reference's loop; the crops themselves are compared, bit-exact."""
    from vtoonify_amd import _lib
    _lib.release_library()
    _no_cv2_no_dlib(monkeypatch)
    _, crops = _clip(tmp_path, n=2)
    seen = []
    loop = cli._cpu_loop

    def spy(opt, model, par, s_w, d_s, source, emit, first_index, bgr):
        def tee():
            for f, p in source:
                seen.append(np.array(f))
                yield f, p
        return loop(opt, model, par, s_w, d_s, tee(), emit, first_index, bgr)

    monkeypatch.setattr(cli, "_cpu_loop", spy)
    rep = cli.main(_args(tmp_path, "src", tmp_path / "o_cpu", extra=("--cpu",)))
    assert _lib._lib is None, "--cpu must not load a library"
    assert len(seen) == 2 and all(np.array_equal(s, c) for s, c in zip(seen, crops))
    assert np.load(rep["output"]).shape == (2, 64, 96, 3)
