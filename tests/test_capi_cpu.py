"""The C-ABI library must build for gfx950 without a GPU, load, and export every symbol include/mccnn.h declares
(no compute calls here -- there is no GPU in the build container)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mccnn_[a-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib_path():
    from mccnn_amd import build
    return build.build()


def test_header_declares_the_expected_surface():
    names = declared_symbols()
    for must in ("mccnn_compute_aabb", "mccnn_num_cells", "mccnn_sort_step1", "mccnn_sort_step2", "mccnn_permute_gather",
                 "mccnn_permute_scatter", "mccnn_transform_indexs", "mccnn_find_neighbors_count",
                 "mccnn_find_neighbors_fill", "mccnn_compute_pdf", "mccnn_poisson_sampling_count",
                 "mccnn_poisson_sampling_fill", "mccnn_spatial_conv_fwd", "mccnn_spatial_conv_bwd", "mccnn_block_size"):
        assert must in names


def test_library_exports_every_declared_symbol(lib_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    missing = [n for n in declared_symbols() if n not in exported]
    assert not missing, missing


def test_binding_covers_header_and_loads(lib_path):
    from mccnn_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_symbols()
    lib = _lib.load()
    assert lib.mccnn_block_size() == 8            # genCompileScript.py:20
    assert lib.mccnn_arch() == b"gfx950"
    assert lib.mccnn_abi_version() >= 1
    assert b"workspace" in lib.mccnn_error_string(-4)
    # host-only entry points (no device access): numCells(scale_inv) known answers, workspace queries
    n = ctypes.c_int(0)
    for r, nc in ((0.1, 10), (0.2, 5), (0.03, 33), (1.9, 1)):
        assert lib.mccnn_num_cells(None, None, 1, r, 1, ctypes.byref(n), None) == 0 and n.value == nc
    assert lib.mccnn_num_cells(None, None, 1, -1.0, 1, ctypes.byref(n), None) == -1
    assert lib.mccnn_sort_step1_workspace_bytes(1000, 2, 10) >= 2 * 1000 * 4 + 1000 * 4
    assert lib.mccnn_sort_step1_workspace_bytes(10, 1 << 20, 1 << 10) == 0     # keys would overflow int32
    assert lib.mccnn_spatial_conv_bwd_workspace_bytes(1000, 1000, 50000, 1, 64, 1) > 50000 * 16


def test_bf16_convolution_entries_refuse_rows_off_the_16_byte_grid(lib_path):
    """The bf16 kernels move 16-byte pieces of the feature / gradient rows, so the two bf16 entry points answer
    MCCNN_E_SHAPE for a row pointer that is not 16-byte aligned (csrc/conv.hip bf16_shape_ok) -- before anything is
    launched or read, which is why made-up addresses and no GPU do here. (The Python ops and the torch extension copy such
    rows into an allocation of their own instead of handing them on: tests/test_gpu_conv_alignment.py.)"""
    from mccnn_amd import _lib
    lib = _lib.load()
    E_SHAPE = -5
    assert b"shape" in lib.mccnn_error_string(E_SHAPE).lower()
    A = 0x7f0000000000          # a made-up, 16-byte aligned address: never dereferenced by the calls below
    p = [A + 0x10000 * k for k in range(32)]
    n = m = 64
    e, fin = 256, 16

    def fwd(feats, out):
        return lib.mccnn_spatial_conv_fwd_bf16(p[0], feats, *p[2:15], n, m, e, fin, 1, 0.1, 0, 1, out, p[16], 1 << 20, None)

    def bwd(feats, og, fg):
        return lib.mccnn_spatial_conv_bwd_bf16(p[0], feats, *p[2:15], og, n, m, e, fin, 1, 0.1, 0, 1, p[17], p[18], fg,
                                               *p[20:26], p[16], 1 << 20, None)

    for d in (2, 4, 8):
        assert fwd(p[1] + d, p[15]) == E_SHAPE and fwd(p[1], p[15] + d) == E_SHAPE
        assert bwd(p[1] + d, p[19], p[26]) == E_SHAPE and bwd(p[1], p[19] + d, p[26]) == E_SHAPE
        assert bwd(p[1], p[19], p[26] + d) == E_SHAPE


def _code_objects(lib_path, tmp_path):
    """llvm-objdump --offloading EXTRACTS the bundles next to its input: work on a copy in a scratch directory.
    -> (objdump's text, paths of the extracted gfx950 code objects)"""
    import shutil
    copy = os.path.join(str(tmp_path), os.path.basename(lib_path))
    shutil.copy(lib_path, copy)
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", copy], capture_output=True, text=True,
                         cwd=str(tmp_path))
    cos = sorted(os.path.join(str(tmp_path), f) for f in os.listdir(str(tmp_path)) if f.endswith("gfx950"))
    return out.stdout + out.stderr, cos


def test_register_budget_of_the_hot_kernels(lib_path, tmp_path):
    """Regression guard: the kernels that run at the edge of the register file must not pick up spills unnoticed (an
    extra kernel argument once cost the depth-wise backward sweep three more spilled registers and 16 % of its time;
    nothing but a timing of that one layer showed it). Budgets = what the shipped build uses (kernel descriptors'
    metadata), with a little slack for compiler updates."""
    _, cos = _code_objects(lib_path, tmp_path)
    if not cos:
        pytest.skip("llvm-objdump did not extract the code objects")
    meta = {}
    for co in cos:
        txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
        for blk in txt.split("- .agpr_count")[1:] if "- .agpr_count" in txt else txt.split("  - .")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            scr = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if name and scr:
                meta[name.group(1)] = int(scr.group(1))
    assert meta, "no kernel metadata found"
    budgets = {
        r"dw_bwd_rowsILi[24]ELb[01]E": 16,   # 12: one pair kept around each slice's sweep (44 / 32 before the row id and the lane id were read afresh after it)
        r"dw_fwd_rowsILi[24]E": 0,
        r"f1_bwd_edges": 0, r"f1_fwd_edges": 0,
        r"conv_streamILb0ELi[24]ELb1E": 0,
        r"conv_bwd_mfmaILb0ELi[24]ELb1E": 0,  # the depth-wise streaming backward (COOP)
        r"conv_bwd_mfmaILb1ELi3ELb0E": 40,     # combin layers with 2..4 input features: 36 since conv.hip is built without SLP (60 before)
    }
    for pat, limit in budgets.items():
        hits = {k: v for k, v in meta.items() if re.search(pat, k)}
        assert hits, pat
        for k, v in hits.items():
            assert v <= limit, "%s: %d bytes of scratch per lane (budget %d)" % (k, v, limit)


def test_code_object_is_gfx950_only(lib_path, tmp_path):
    txt, _ = _code_objects(lib_path, tmp_path)
    if "gfx" not in txt:
        out = subprocess.check_output(["strings", lib_path], text=True)
        txt = "\n".join(l for l in out.splitlines() if "amdgcn-amd-amdhsa" in l)
    archs = set(re.findall(r"gfx[0-9a-f]+", txt))
    assert archs == {"gfx950"}, archs


def test_product_package_never_touches_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load the oracle."""
    pkg = os.path.join(ROOT, "mccnn_amd")
    bad = re.compile(r"(^|\s)(import\s+oracle|from\s+oracle)|liboracle|orc_[a-z]|oracle/|oracle\.oracle")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, f)).read()
                assert not bad.search(src), os.path.join(dp, f)


def test_environment_switches_are_a_handful():
    """The product package reads FOUR documented path switches, the MCCNN_DEBUG list and the two A/B build variables of
    mccnn_amd.build -- nothing else (csrc/debug_opts.h, mccnn_amd/_env.py)."""
    import glob
    import re
    names = set()
    for f in glob.glob(os.path.join(ROOT, "mccnn_amd", "*.py")) + glob.glob(os.path.join(ROOT, "mccnn_amd", "csrc", "*")):
        if not os.path.isfile(f):
            continue
        txt = open(f, errors="ignore").read()
        names |= set(re.findall(r'(?:getenv|environ\.get|environ\[)\(?\s*"(MCCNN_[A-Z0-9_]+)"', txt))
        names |= set("MCCNN_" + n for n in re.findall(r'_env\.flag\("([A-Z0-9_]+)"', txt) + re.findall(r'\bflag\("([A-Z0-9_]+)"\)', txt))
    assert names <= {"MCCNN_NATIVE", "MCCNN_TORCH_EXT", "MCCNN_ROW_KERNELS", "MCCNN_GEO_PREFETCH", "MCCNN_DEBUG", "MCCNN_LIB_NAME",
                     "MCCNN_EXTRA_FLAGS"}, sorted(names)


def test_debug_list_parser(monkeypatch):
    """mccnn_amd/_env.py: the four path switches and the MCCNN_DEBUG list (bare key = 1, typed by the default)."""
    import importlib
    monkeypatch.setenv("MCCNN_DEBUG", "small_off, plan_min_l=16 ,ecap_scale=0.5,fuse_sort=0,geo_trace")
    monkeypatch.setenv("MCCNN_NATIVE", "0")
    monkeypatch.delenv("MCCNN_TORCH_EXT", raising=False)
    from mccnn_amd import _env
    env = importlib.reload(_env)
    try:
        assert env.debug("small_off", 0) == 1 and env.debug("plan_min_l", 4) == 16
        assert env.debug("ecap_scale", 1.0) == 0.5 and env.debug("fuse_sort", True) is False and env.debug("geo_trace", False) is True
        assert env.debug("absent", 7) == 7 and env.debug("absent", "x") == "x"
        assert env.flag("NATIVE") is False and env.flag("TORCH_EXT") is True
    finally:
        monkeypatch.delenv("MCCNN_DEBUG")
        monkeypatch.delenv("MCCNN_NATIVE")
        importlib.reload(_env)


def test_rowplan_bound_covers_every_edge_count():
    """mccnn_rowplan_bound(rows, e_cap): buffer and workspace sizes that hold for EVERY list of up to e_cap edges -- what a
    caller allocates before the true total is known (plans prebuilt on helper threads). The piece length L is a step
    function of (rows, e) with several regimes (single-workgroup form with pieces of <= 16 edges, mid-size lists, large
    lists): checked against mccnn_rowplan_buffer / _build_workspace_bytes on random shapes. Host arithmetic only."""
    import ctypes as C
    import numpy as np
    from mccnn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(5)
    offs = (C.c_longlong * 6)()
    for _ in range(300):
        rows = int(rng.choice([1, 7, 73, 318, 1273, 3000, 3100, 4096, 5627, 16000, 20000, 100000, 800000]))
        e_cap = int(rows * rng.choice([0.5, 3, 8, 33, 60, 400]) + rng.integers(0, 1000))
        for tr in (0, 1):
            b, w = C.c_longlong(0), C.c_longlong(0)
            assert lib.mccnn_rowplan_bound(rows, e_cap, tr, C.byref(b), C.byref(w)) == 0
            for e in sorted(set([1, e_cap, e_cap // 2, e_cap // 7 + 1] + [int(x) for x in rng.integers(1, e_cap + 1, 6)])):
                total, cap, srows, S = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0), C.c_int(0)
                assert lib.mccnn_rowplan_buffer(rows, e, offs, C.byref(total), C.byref(S), C.byref(cap), C.byref(srows)) == 0
                assert total.value <= b.value, (rows, e, e_cap, tr, total.value, b.value)
                assert lib.mccnn_rowplan_build_workspace_bytes(rows, e, tr) <= w.value, (rows, e, e_cap, tr)


def test_debug_list_parser_of_the_library(tmp_path):
    """csrc/debug_opts.h (the C++ side of the MCCNN_DEBUG list): bare keys, values, blanks, a key that is a prefix of another."""
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    src = tmp_path / "t.cpp"
    src.write_text('#include "debug_opts.h"\n#include <cstdio>\nint main() { printf("%d %d %d %d %g\\n", mccnn::debug_int("small_off", 0), '
                   'mccnn::debug_int("plan_min_l", 4), mccnn::debug_int("absent", 7), mccnn::debug_int("plan_min", 9), '
                   'mccnn::debug_float("ecap_scale", 1.0)); }\n')
    exe = tmp_path / "t"
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "mccnn_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], env=dict(os.environ, MCCNN_DEBUG="small_off, plan_min_l=16 ,ecap_scale=0.5"), capture_output=True, text=True)
    assert out.stdout.split() == ["1", "16", "7", "9", "0.5"]


def test_debug_keys_one_table_and_unknown_keys_are_reported(tmp_path):
    """ONE table of MCCNN_DEBUG keys: kDebugKeys (csrc/debug_opts.h) == KNOWN_KEYS (mccnn_amd/_env.py); every key that any
    source file queries is in it and every key in it is queried by some source file (no dead entries); a key that is not
    in it is reported on stderr by both sides (a misspelt A/B switch used to be ignored silently -- the void-A/B failure
    mode of round 5)."""
    import glob
    import re
    import shutil
    import subprocess
    import sys
    from mccnn_amd import _env
    hdr = open(os.path.join(ROOT, "mccnn_amd", "csrc", "debug_opts.h")).read()
    body = hdr[hdr.index("#define MCCNN_DEBUG_KEYS"):hdr.index("static const char* const kDebugKeys")]
    ckeys = re.findall(r'"([a-z0-9_]+)"', body)
    assert ckeys == list(_env.KNOWN_KEYS) and len(set(ckeys)) == len(ckeys)
    used = set()
    for f in glob.glob(os.path.join(ROOT, "mccnn_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "mccnn_amd", "*.py")):
        if os.path.isfile(f):
            txt = open(f, errors="ignore").read()
            used |= set(re.findall(r'debug_(?:int|float|opt)\("([a-z0-9_]+)"', txt))
            used |= set(re.findall(r'_env\.debug\(\s*"([a-z0-9_]+)"', txt))
    assert used <= set(ckeys), sorted(used - set(ckeys))
    assert set(ckeys) <= used, sorted(set(ckeys) - used)
    # the Python side reports an unknown key ...
    r = subprocess.run([sys.executable, "-c", "from mccnn_amd import _env; print(_env.debug('small_off', 0))"], cwd=ROOT,
                       env=dict(os.environ, MCCNN_DEBUG="small_off,plan_smal=8192"), capture_output=True, text=True)
    assert r.stdout.strip() == "1" and "plan_smal" in r.stderr and "small_off" not in r.stderr
    # ... and so does the library's parser
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    src = tmp_path / "t.cpp"
    src.write_text('#include "debug_opts.h"\nint main() { return mccnn::debug_int("small_off", 0) + mccnn::debug_int("plan_small", 4096) == 4097 ? 0 : 1; }\n')
    exe = tmp_path / "t"
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "mccnn_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], env=dict(os.environ, MCCNN_DEBUG="small_off, plan_smal=8192 ,nw_lean=1"), capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr.count("not known") == 1 and "plan_smal" in out.stderr


def test_library_issues_no_memsets():
    """Round 6: clears ride on kernels of the chain they belong to (csrc/common.h ClearSpan) -- a hipMemsetAsync is a launch
    of its own (13-61 `fillBufferAligned` per step of the BASELINE configurations in round 5). None may come back."""
    import glob
    import re
    bad = re.compile(r"\bhipMemset\w*\s*\(")
    for f in sorted(glob.glob(os.path.join(ROOT, "mccnn_amd", "csrc", "*"))):
        if os.path.isfile(f):
            src = re.sub(r"//[^\n]*", "", open(f, errors="ignore").read())
            assert not bad.search(src), f


def test_library_has_no_unresolved_symbols_of_its_own(lib_path):
    """A shared-library link does not report undefined symbols: a function declared in a header (csrc/batch.h) and defined
    with another linkage only fails when the library is LOADED -- on the GPU box. Every undefined dynamic symbol of the
    library in the package's namespace (mccnn::, mccnn_*) is such a mistake."""
    import shutil
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    if not os.path.exists(nm) and not shutil.which(nm):
        pytest.skip("no nm")
    out = subprocess.run([nm, "-D", "--undefined-only", lib_path], capture_output=True, text=True, check=True).stdout
    own = [l.split()[-1] for l in out.splitlines() if l.split() and (l.split()[0] == "U") and ("mccnn" in l.split()[-1])]
    assert not own, own
