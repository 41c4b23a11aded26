"""tools/smooth_parsing_map_amd.py: the reference's option table, and the golden clip as .npy through the command line --
the file name, shape and dtype the reference writes (smooth_parsing_map.py:169-170), the content ParsingSmoother gives.
The source classes moved to tools/frame_sources.py and style_transfer_amd.py still exposes them.
tools/style_transfer_amd.py --smooth_window: one command equals the two-step run byte for byte, two gloo ranks equal one
process, and --smooth_window 0 changes nothing (mirroring tests/test_style_transfer_cli.py; 32 x 32 frames and 2 RAFT
iterations keep the emulation affordable -- equality between runs does not depend on the count)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, load_keys

sys.path.insert(0, os.path.join(REPO, "tools"))
import smooth_parsing_map_amd as cli  # noqa: E402

REFERENCE_OPTIONS = {   # smooth_parsing_map.py:21-27: dest -> (type, default)
    "window_size": (int, 5), "faceparsing_path": (str, "./checkpoint/faceparsing.pth"),
    "raft_path": (str, "./checkpoint/raft-things.pth"), "video_path": (str, None), "output_path": (str, "./output/"),
}


def test_option_table_is_the_references():
    mine = {a.dest: (a.type, a.default) for a in cli.build_parser()._actions if a.dest != "help"}
    for k, v in REFERENCE_OPTIONS.items():
        assert mine[k] == v, k
    assert {"precision", "frame_order", "max_frames", "seed"} <= set(mine)


def test_sources_are_shared_not_copied():
    import frame_sources
    import style_transfer_amd
    for name in ("NpySource", "DirSource", "Cv2Source", "open_source"):
        assert getattr(style_transfer_amd, name) is getattr(frame_sources, name)
    assert cli.open_source is frame_sources.open_source


def test_golden_clip_through_the_command_line(dev, tmp_path, monkeypatch):
    from vtoonify_amd import smooth, synth
    from vtoonify_amd.bisenet import BiSeNetEngine
    from vtoonify_amd.raft import RaftEngine
    monkeypatch.setenv("VT_BATCH_EXACT", "1")
    d, _ = load_golden("smooth_stream.npz")
    frames, window = d["frames"], int(d["cfg"][0])
    np.save(tmp_path / "myclip.npy", frames)
    rep = cli.main(["--video_path", str(tmp_path / "myclip.npy"), "--output_path", str(tmp_path / "out"), "--window_size",
                    str(window), "--raft_path", "synthetic", "--faceparsing_path", "synthetic", "--frame_order", "rgb",
                    "--chunk", "2"], device=dev)
    assert rep["output"] == str(tmp_path / "out" / "myclip_parsingmap.npy") and rep["frames"] == 7
    got = np.load(rep["output"])
    assert got.shape == (7, 19, 64, 64) and got.dtype == np.float32 and rep["peak_slots"] == 2 * window + 1
    raft = RaftEngine(synth.synth_state_dict(load_keys("raft"), 0), torch.float32, dev)
    bise = BiSeNetEngine(synth.synth_state_dict(load_keys("bisenet"), 0), 19, torch.float32, dev)
    sm = smooth.ParsingSmoother(raft, bise, window, bgr=False)
    want = torch.cat(list(sm.smooth([torch.from_numpy(frames)])), 0).cpu().numpy()
    assert np.array_equal(got, want)
    with pytest.raises(SystemExit):
        cli.main(["--output_path", str(tmp_path / "out")], device=dev)


# ------------------------------------------------------------------------------- style_transfer_amd.py --smooth_window
import socket  # noqa: E402
import subprocess  # noqa: E402

import style_transfer_amd as st  # noqa: E402


def _clip(tmp_path, n=5, H=32, W=32):
    d, _ = load_golden("smooth_stream.npz")
    frames = np.ascontiguousarray(d["frames"][:n, 8:8 + H, 16:16 + W])
    np.save(tmp_path / "clip.npy", frames)
    np.save(tmp_path / "code.npy", np.random.default_rng(3).standard_normal((1, 18, 512)).astype(np.float32))
    return frames


def _style_args(tmp_path, out, extra=()):
    return ["--content", str(tmp_path / "clip.npy"), "--video", "--intrinsic_code", str(tmp_path / "code.npy"), "--ckpt",
            "synthetic", "--backbone", "toonify", "--output_path", str(out), "--batch_size", "2", "--depth", "2",
            "--precision", "bf16", "--frame_order", "rgb", *extra]


SMOOTH = ("--smooth_window", "2", "--smooth_iters", "2", "--raft_path", "synthetic", "--faceparsing_path", "synthetic")


def test_style_options_added_with_smoothing_off_by_default():
    opt = st.parse([])
    assert opt.smooth_window == 0 and opt.raft_path == "./checkpoint/raft-things.pth"


def test_smooth_window_equals_the_two_step_run(dev, tmp_path):
    _clip(tmp_path)
    rep = cli.main(["--video_path", str(tmp_path / "clip.npy"), "--output_path", str(tmp_path / "maps"), "--window_size", "2",
                    "--iters", "2", "--raft_path", "synthetic", "--faceparsing_path", "synthetic", "--frame_order", "rgb"],
                   device=dev)
    two = np.load(st.main(_style_args(tmp_path, tmp_path / "o2", ("--parsing_map_path", rep["output"])), device=dev)["output"])
    one = np.load(st.main(_style_args(tmp_path, tmp_path / "o1", SMOOTH), device=dev)["output"])
    assert one.shape == two.shape == (5, 128, 128, 3) and one.dtype == np.uint8
    assert one.tobytes() == two.tobytes()
    assert not os.path.exists(tmp_path / "o1" / "clip_parsingmap.npy")          # nothing on disk in between
    with pytest.raises(SystemExit):
        st.main(_style_args(tmp_path, tmp_path / "o3", SMOOTH + ("--parsing_map_path", rep["output"])), device=dev)


_WORKER = """
import os, sys
sys.path.insert(0, os.environ["VT_REPO"]); sys.path.insert(0, os.path.join(os.environ["VT_REPO"], "tests"))
sys.path.insert(0, os.path.join(os.environ["VT_REPO"], "tools"))
from emu import build_emu
from vtoonify_amd import _lib
_lib.use_library(build_emu.build())
import style_transfer_amd as cli
rep = cli.main(sys.argv[1:], device="cpu", backend="gloo")
print("rank", rep["rank"], "shard", rep["shard"], "ok")
"""


def test_two_ranks_smooth_like_one_process(tmp_path):
    from emu import build_emu
    from vtoonify_amd import _lib
    _lib.use_library(build_emu.build())
    _clip(tmp_path)
    one = np.load(st.main(_style_args(tmp_path, tmp_path / "out1", SMOOTH), device="cpu")["output"])
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), VT_REPO=REPO, OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, str(script)] + _style_args(tmp_path, tmp_path / "out2", SMOOTH),
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=1800)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o}"
    assert "shard (0, 3)" in outs[0] and "shard (3, 5)" in outs[1]       # each shard's window crosses the cut
    two = np.load(tmp_path / "out2" / "clip_vtoonify_t.npy")
    assert two.shape == one.shape and np.array_equal(two, one), "sharded smoothing must write the one-process video"


def test_smooth_window_zero_changes_nothing(tmp_path):
    """The input of tests/test_style_transfer_cli.py::test_one_process_video_equals_frame_by_frame: with --smooth_window 0
    the driver writes what it writes without the flag, which is the frame-by-frame result of that test's oracle."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import frames_oracle as FO
    import test_style_transfer_cli as T
    from vtoonify_amd import synth
    from vtoonify_amd.vtoonify import VToonify
    T._emu()
    frames, maps = T._clip(tmp_path, n=3)
    base = np.load(st.main(T._args(tmp_path, tmp_path / "a"), device="cpu")["output"])
    off = np.load(st.main(T._args(tmp_path, tmp_path / "b", extra=("--smooth_window", "0")), device="cpu")["output"])
    assert off.tobytes() == base.tobytes()
    m = VToonify(backbone="toonify", compute_dtype=torch.bfloat16)
    m.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 0))
    s_w = m.zplus2wplus(torch.from_numpy(np.load(tmp_path / "code.npy")))
    for i in range(3):
        y = m(torch.from_numpy(FO.pack_inputs(frames[i][None], maps[i][None])), s_w, d_s=None)
        assert np.array_equal(off[i], FO.tensor2cv2(y[0].float().numpy())), i
