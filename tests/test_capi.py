"""libm3d.so loads on the host and exports every entry point of include/m3d.h
(no compute calls: there is no GPU in the CPU suite)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "m3d.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(m3d_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import m3d._lib as lib
    L = lib.load()
    syms = header_symbols()
    assert len(syms) >= 20
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing
    # and the Python binding declares a signature for each of them
    assert sorted(lib.EXPORTED) == syms


def test_error_string_and_version():
    import m3d._lib as lib
    L = lib.load()
    assert L.m3d_abi_version() == 3
    assert isinstance(L.m3d_last_error(), bytes)


def test_invalid_arguments_are_rejected_without_touching_the_gpu():
    import m3d._lib as lib
    L = lib.load()
    rc = L.m3d_nms3d(None, None, 10, 5, 1.5, 0, None, None, None, 0, None)
    assert rc == -1 and b"iou_threshold" in L.m3d_last_error()
    rc = L.m3d_crop_and_resize3d_fwd(None, 1, 4, 4, 4, 1, None, None, 1, 0, 2, 2, 0, 0.0, None, None)
    assert rc == -1 and b"crop dimensions must be positive" in L.m3d_last_error()
    rc = L.m3d_crop_and_resize3d_fwd(None, 1, 4, 4, 4, 1, None, None, 1, 2, 2, 2, 7, 0.0, None, None)
    assert rc == -1 and b"method" in L.m3d_last_error()


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from m3d import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.crop_and_resize_3d(torch.zeros(1, 4, 4, 4, 1), torch.zeros(1, 6),
                               torch.zeros(1, dtype=torch.int32), (2, 2, 2))
    with pytest.raises(ValueError, match="GPU"):
        ops.non_max_suppression_3d(torch.zeros(3, 6), torch.zeros(3), 2, 0.5)


def test_tf_binding_matches_header():
    """integration/tf/m3d_tf_ops.cc (the TF OpKernel binding, INTEGRATION.md
    §2a; not buildable here: TF is absent) calls only declared, exported entry
    points, with the declared argument count, and registers the wheel's four
    op names on DEVICE_GPU."""
    import m3d._lib as lib
    src = open(os.path.join(ROOT, "integration", "tf", "m3d_tf_ops.cc")).read()
    hdr = open(os.path.join(ROOT, "include", "m3d.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = lib.load()

    def nargs(text, name):
        i = text.index(name + "(") + len(name) + 1
        depth, n, j = 1, 1, i
        while depth:
            c = text[j]
            depth += c == "(" or -(c == ")")
            n += c == "," and depth == 1
            j += 1
        return n if text[i:j - 1].strip() not in ("", "void") else 0

    called = sorted(set(re.findall(r"\b(m3d_[a-z0-9_]+)\s*\(", src)) - {"m3d_status"})
    assert "m3d_nms3d" in called and "m3d_crop_and_resize3d_fwd" in called
    for name in called:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(L, name), name
        assert nargs(re.sub(r"//[^\n]*", "", src), name) == nargs(hdr, name), name
    for op in ("CropAndResize3D", "CropAndResize3DGradImage", "CropAndResize3DGradBoxes",
               "NonMaxSuppression3D"):
        assert f'REGISTER_OP("{op}")' in src
        assert re.search(r'Name\("' + op + r'"\)\.Device\(DEVICE_GPU\)', src), op


def test_tf_op_defs_match_the_wheel():
    """Every REGISTER_OP of the TF binding declares exactly the wheel's op-def:
    the same .Input / .Output / .Attr specs in the same order, compared with
    the strings extracted statically from the reference's vendored op
    libraries (tests/golden/wheel_opdefs.json, tests/golden/extract_opdefs.py)
    -- e.g. CropAndResize3D's third input is `box_index`, its grad ops'
    `box_ind`."""
    import json
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "wheel_opdefs.json")))
    src = open(os.path.join(ROOT, "integration", "tf", "m3d_tf_ops.cc")).read()
    src = re.sub(r"//[^\n]*", "", src)
    assert len(want) == 4
    for op, d in want.items():
        i = src.index(f'REGISTER_OP("{op}")')
        j = src.index(".SetShapeFn", i)
        got = re.findall(r'\.(?:Input|Output|Attr)\("([^"]*)"\)', src[i:j])
        assert got == d["specs"], (op, got, d["specs"])


def test_runtime_switches_are_few_and_tested():
    """The product reads its environment only where a test drives the switch
    (VERDICT r3 item 8, r4 weak 7): every kernel-variant choice is a
    compile-time M3D_TUNE_* constant (csrc/common.h; A/B builds via make ab) and
    every host-side path choice a module constant of m3d (tests monkeypatch
    them).  Scanned: the library sources and the host package."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pat = re.compile(r'(?:getenv|environ\.get|environ\[)\(?\s*"(M3D_\w+)"')
    names = {}
    for f in glob.glob(os.path.join(root, "3d-mask-r-cnn_amd", "csrc", "*")) + \
            glob.glob(os.path.join(root, "3d-mask-r-cnn_amd", "m3d", "*.py")):
        for n in pat.findall(open(f).read()):
            names.setdefault(n, []).append(os.path.basename(f))
    assert set(names) <= {"M3D_OPERAND_LIMIT", "M3D_LIB_FILE", "M3D_DIST_TIMEOUT"}, names
    tests_text = "".join(open(f).read() for f in glob.glob(os.path.join(root, "tests", "*.py"))
                         if not f.endswith("test_capi.py"))
    for n in names:
        assert n in tests_text, f"{n} is read by the product but no test drives it"


def test_no_process_wide_mutable_state():
    """libm3d is reentrant: its data objects
    are the toolchain's / HIP runtime's own (code-object handles, init flags)
    and two thread-locals (the error text, the det scope of the running call)
    -- no mode or cache shared between calls (the deterministic target is a
    per-call m3d_det_t, the fork events the caller's).  The one exception is the
    test-only operand bound, read from the environment once
    (M3D_OPERAND_LIMIT)."""
    import subprocess
    import m3d._lib as lib
    out = subprocess.run(["readelf", "-sW", "--demangle", lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    tls, bad = [], []
    for line in out.splitlines():
        f = line.split()
        if len(f) < 8 or f[3] not in ("OBJECT", "TLS") or f[6] == "UND":
            continue
        name = " ".join(f[7:])
        if f[3] == "TLS":
            tls.append(name)
            continue
        if name.startswith(("__hip_", "__do_init.", "__do_fini.", "__init", "__fini", "__dso_handle",
                            "__EH_FRAME_LIST", "DW.ref.", "__TMC_END__", "_DYNAMIC", "_GLOBAL_OFFSET_TABLE_")):
            continue
        if "op_lim()::v" in name or name == "guard variable for":
            continue
        if name.endswith(")") and "(" in name:
            continue                                    # a kernel's host handle (its signature)
        bad.append(name)
    assert not bad, bad
    assert sorted(tls) == ["m3d::g_err", "m3d::t_det"], tls


def test_det_argument_is_validated():
    """A deterministic target that is on but has no / a short / a misaligned
    scratch is M3D_EINVAL before anything is enqueued (no GPU touched)."""
    import m3d._lib as lib
    L = lib.load()
    for d in (lib.Det(1, None, 1 << 20), lib.Det(1, 1 << 20, 64), lib.Det(1, (1 << 20) + 4, 1 << 20)):
        rc = L.m3d_gemm_wgrad_f32(None, None, None, 1, 4, 4, 4, ctypes.addressof(d), None)
        assert rc == -1 and b"det->scratch" in L.m3d_last_error()


def test_rpn_targets_rejects_atss_topk_below_one():
    """ATSS_TOPK < 1 would reach mu = sum / 0 in atss_kernel: both entry points
    return M3D_EINVAL before anything is enqueued (no GPU touched); the same
    call with ATSS_TOPK = 1 gets past that check, to the workspace one."""
    import m3d._lib as lib
    L = lib.load()
    sd = (lib.c_f * 6)(*([0.1] * 6))
    for fn in (L.m3d_rpn_targets, L.m3d_rpn_targets_async):
        for topk in (0, -3):
            rc = fn(None, 100, None, 2, 0.3, 0.1, 64, 0.5, topk, 4, sd, 0, None, None, 100, None, 0, None, None)
            assert rc == -1 and b"ATSS_TOPK" in L.m3d_last_error()
        rc = fn(None, 100, None, 2, 0.3, 0.1, 64, 0.5, 1, 4, sd, 0, None, None, 100, None, 0, None, None)
        assert rc == -1 and b"workspace too small" in L.m3d_last_error()


def test_wino_dgrad_workspace_follows_the_call_tile():
    """a data-gradient call's tile_y sets its U / M layout, so its
    workspace check must use that tile, not the library default.  The
    workspace function covers both tiles; a tile_y = 2 call with a workspace
    sized for tile_y = 4 (fewer tiles x points) is rejected before any launch."""
    import m3d._lib as lib
    L = lib.load()
    for (B, H, W, D, C1, C2) in ((1, 32, 32, 128, 256, 512), (1, 8, 8, 8, 64, 64), (2, 16, 16, 32, 128, 128)):
        nb = L.m3d_conv3d_wino_workspace_bytes(B, H, W, D, D, C1, C2)
        n2 = L.m3d_conv3d_wino_dgrad_workspace_bytes(B, H, W, D, D, C1, C2, 2)
        n4 = L.m3d_conv3d_wino_dgrad_workspace_bytes(B, H, W, D, D, C1, C2, 4)
        assert n2 > 0 and n4 > 0 and nb >= max(n2, n4)
        assert L.m3d_conv3d_wino_dgrad_workspace_bytes(B, H, W, D, D, C1, C2, 3) == 0
        small, big = sorted((n2, n4))
        ty_big = 2 if n2 > n4 else 4
        fake = ctypes.c_void_p(0x1000)
        rc = L.m3d_conv3d_bwd_data_wino_vy(fake, fake, B, H, W, D, C1, C2, D, 1, fake, 0, fake, small, 0,
                                           ty_big, None)
        assert rc == -1 and b"workspace too small" in L.m3d_last_error()
        rc = L.m3d_conv3d_bwd_data_wino_vy(fake, fake, B, H, W, D, C1, C2, D, 1, fake, 0, fake, big, 0, 3, None)
        assert rc == -1 and b"tile_y" in L.m3d_last_error()


def test_compile_time_switches_are_few():
    """the refuted and measured-slower kernel variants are
    deleted, not parked behind switches: at most 25 M3D_TUNE_* constants."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = set()
    for f in glob.glob(os.path.join(root, "3d-mask-r-cnn_amd", "csrc", "*")):
        names |= set(re.findall(r"\bM3D_TUNE_[A-Z0-9_]+", open(f).read()))
    assert len(names) <= 25, sorted(names)
