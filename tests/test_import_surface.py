"""Drop-in import surface: the mirror package `model` resolves every import target of the
reference's scripts (style_transfer.py, util.py, smooth_parsing_map.py) to vtoonify_amd.

Runs in a subprocess: the mirror package is called `model`, like the reference's, and must not leak into the
other tests' sys.modules."""
import os
import subprocess
import sys
import textwrap

from conftest import REPO


def test_mirror_package_re_exports_without_the_reference():
    """The mirror alone (no reference on the path): the six import targets resolve to vtoonify_amd."""
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {REPO!r})
        from model.vtoonify import VToonify
        from model.bisenet.model import BiSeNet
        from model.stylegan.op import FusedLeakyReLU, fused_leaky_relu, upfirdn2d, conv2d_gradfix
        from model.stylegan.op.conv2d_gradfix import conv2d, conv_transpose2d, no_weight_gradients
        from model.encoder.encoders.psp_encoders import GradualStyleEncoder
        from model.raft.core.raft import RAFT                     # smooth_parsing_map.py:12
        import vtoonify_amd.op, vtoonify_amd.vtoonify, vtoonify_amd.psp, vtoonify_amd.bisenet, vtoonify_amd.raft
        assert RAFT is vtoonify_amd.raft.RAFT
        assert VToonify is vtoonify_amd.vtoonify.VToonify and BiSeNet is vtoonify_amd.bisenet.BiSeNet
        assert GradualStyleEncoder is vtoonify_amd.psp.GradualStyleEncoder
        assert conv2d_gradfix is vtoonify_amd.op.conv2d_gradfix and conv2d is conv2d_gradfix.conv2d
        assert upfirdn2d is vtoonify_amd.op.upfirdn2d
        conv2d_gradfix.enabled = False      # module globals are the implementation's own
        assert vtoonify_amd.op.conv2d_gradfix.enabled is False
        print("MIRROR_OK")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0 and "MIRROR_OK" in r.stdout, r.stdout + r.stderr
