"""CPU checks of the drop-in boundary: the gfx950 library builds, loads and exports every
symbol declared in include/vtoonify_amd.h; the loader fails loudly when it is missing; the
Python op surface has the reference's signatures.  No kernel is launched here."""
import ctypes
import inspect
import json
import os
import re
import sys

import pytest

from conftest import REPO
from vtoonify_amd import _lib


def _declared():
    src = open(os.path.join(REPO, "include", "vtoonify_amd.h")).read()
    return sorted(set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_agree():
    assert sorted(_lib.EXPORTED_SYMBOLS) == _declared()


def test_gfx950_library_exports_every_symbol():
    from vtoonify_amd import build
    path = build.build(verbose=False)  # hipcc cross-compiles without a GPU
    lib = ctypes.CDLL(path)
    for name in _declared():
        assert hasattr(lib, name), f"{name} not exported by {path}"
    lib.vt_abi_version.restype = ctypes.c_int
    assert lib.vt_abi_version() == _lib.ABI_VERSION == 5
    lib.vt_build_target.restype = ctypes.c_char_p
    assert lib.vt_build_target() == b"gfx950"


def test_loader_fails_loudly_without_library(tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "DEFAULT_LIB", str(tmp_path / "libvtoonify_amd.so"))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.VtError, match="no CPU fallback"):
        _lib.lib()


def test_cpu_tensors_are_rejected_by_the_product_library():
    import torch
    from vtoonify_amd import build, kernels as K
    _lib.use_library(build.build(verbose=False))
    with pytest.raises(_lib.VtError, match="GPU only"):
        K.fused_bias_act(torch.zeros(1, 2, 3, 3), None, None, 3, 0, 0.2, 1.0)


def test_op_surface_signatures_match_reference():
    from vtoonify_amd import op
    assert [p for p in inspect.signature(op.upfirdn2d).parameters] == ["input", "kernel", "up", "down", "pad"]
    assert [p for p in inspect.signature(op.fused_leaky_relu).parameters] == \
        ["input", "bias", "negative_slope", "scale"]
    assert [p for p in inspect.signature(op.FusedLeakyReLU.__init__).parameters] == \
        ["self", "channel", "bias", "negative_slope", "scale"]
    assert [p for p in inspect.signature(op.conv2d_gradfix.conv2d).parameters] == \
        ["input", "weight", "bias", "stride", "padding", "dilation", "groups"]
    assert [p for p in inspect.signature(op.conv2d_gradfix.conv_transpose2d).parameters] == \
        ["input", "weight", "bias", "stride", "padding", "output_padding", "groups", "dilation"]
    assert op.conv2d_gradfix.enabled is True and op.conv2d_gradfix.weight_gradients_disabled is False
    with op.conv2d_gradfix.no_weight_gradients():
        assert op.conv2d_gradfix.weight_gradients_disabled is True
    m = op.FusedLeakyReLU(7)
    assert list(m.state_dict()) == ["bias"] and m.bias.shape == (7,)
    # against the reference's own signatures (tests/golden/reference_api.json, parsed from its `model.stylegan.op` and
    # CPU twin `op_cpu` by tests/golden/make_golden_api.py): same names and defaults as op, same positions as op_cpu
    with open(os.path.join(REPO, "tests", "golden", "reference_api.json")) as f:
        api = json.load(f)
    for name, ref in api["op"].items():
        obj = op
        for part in name.split("."):
            obj = getattr(obj, part)
        params = inspect.signature(obj).parameters
        mine = {"params": list(params), "defaults": {k: json.loads(json.dumps(p.default)) for k, p in params.items()
                                                     if p.default is not inspect.Parameter.empty}}
        assert mine == ref, name
        twin = api["op_cpu"][name]
        assert twin["params"][1:] == ref["params"][1:] and twin["defaults"] == ref["defaults"], name


def test_vtoonify_signature_and_state_dict_schema():
    import torch
    from conftest import load_keys
    from vtoonify_amd.vtoonify import VToonify
    sig = inspect.signature(VToonify.forward)
    assert list(sig.parameters) == ["self", "x", "style", "d_s", "return_mask", "return_feat"]
    ctor = inspect.signature(VToonify.__init__).parameters
    for name, default in [("in_size", 256), ("out_size", 1024), ("img_channels", 3), ("style_channels", 512),
                          ("num_mlps", 8), ("channel_multiplier", 2), ("num_res_layers", 6),
                          ("backbone", "dualstylegan")]:
        assert ctor[name].default == default
    for tag, bb, n in (("D", "dualstylegan", 399), ("T", "toonify", 229)):
        want = load_keys(tag)
        got = {k: tuple(v.shape) for k, v in VToonify(backbone=bb).state_dict().items()}
        assert len(want) == n and got == want


def test_hot_kernels_do_not_spill():
    """Registers / scratch of every kernel of the built gfx950 objects (tools/kernel_resources.py).  A spill in an
    unrolled epilogue is invisible in the source: two extra activation branches in conv_finish put 272 bytes of scratch
    per lane into the 128-channel tile kernels and cost the 256x128 instance 35 % (round 2).  Only the kernels that are
    deliberately capped at 256 registers (`__launch_bounds__(T, 2)`) may keep a few cold
    values in scratch."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from vtoonify_amd import build
    build.build(verbose=False)
    import kernel_resources
    table = kernel_resources.kernel_table()
    assert len(table) > 100
    # (conv_patchq_kernel<256x128>: 14 loop-invariant values written in the prologue and read back in the epilogue -- none inside
    # the K loop -- because the persistent tile loop keeps the epilogue's operands and the loader's offsets alive together)
    capped = ("conv_upblur_kernel", "conv_patchq_kernel")
    bad = {k: v["scratch"] for k, v in table.items()
           if v["scratch"] > (128 if any(c in k for c in capped) else 0)}
    assert not bad, bad

# every environment switch the product reads, as DESIGN.md section 8 documents them (49 switches, most of
# them lost A/B arms, were a correctness surface nobody tested; round 4 deleted the dead arms)
DOCUMENTED_SWITCHES = {
    # meaning for a user of the package
    "VTOONIFY_AMD_DTYPE", "VT_BATCH_EXACT", "VT_MAX_PLANS", "VT_TILE_HINTS", "VT_GRAPH_FIRST", "VT_STYLE_GATE", "VT_PATCH_PIPE",
    "VT_FULLKW", "VT_RAFT_GRAPH",
    # test hooks: force a kernel form that the heuristics only choose at sizes a CPU-emulated test cannot afford
    "VT_C32_BLOCKS", "VT_UPBLUR_WGS", "VT_PATCHW_WGS", "VT_UPBLUR_TALL", "VT_UPBLUR_P8", "VT_UPBLUR_DB", "VT_UPBLUR_ROWS", "VT_UPBLUR_FLAT", "VT_UPBLUR_FLAT_CN",
    "VT_FULLKW_MIN_G", "VT_FULLKW_G",
    "VT_SPLITK_IN_LAUNCH", "VT_GATE_LOADER",
}


def test_product_reads_only_documented_switches():
    import re
    found = set()
    root = os.path.join(REPO, "vtoonify_amd")
    for dp, _, files in os.walk(root):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp")):
                src = open(os.path.join(dp, f), errors="ignore").read()
                found |= set(re.findall(r'getenv\("(VT[A-Z0-9_]*)"\)', src))
                found |= set(re.findall(r'environ(?:\.get\(|\[)"(VT[A-Z0-9_]*)"', src))
    assert found <= DOCUMENTED_SWITCHES, sorted(found - DOCUMENTED_SWITCHES)
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    missing = [s for s in sorted(found) if s not in design]
    assert not missing, f"switches read by the product but not in DESIGN.md: {missing}"
