"""The rows / streaming rule lives in the library alone (rows_shape() in csrc/exec.hip, asked through mccnn_conv_rows_shape) and
one route record per layer decides what mccnn_conv_prepare / _forward / _backward do. Without a GPU:
  1. the query against the rule MCConvModule._rows_shape stated itself before it asked the library (copied literally below),
     on a lattice around every threshold -- all edge counts <= 2^24, where its double comparison e / rows >= 16 and the
     library's float one agree exactly;
  2. MCConvModule._rows_shape on host tensors of those shapes gives the query's answers, behind its two switches
     (ROW_KERNELS, bit 2 of debug_conv_impl's mask);
  3. UNSORTED_MAX_POINTS is the library's value;
  4. header, binding and library hold the two entries and the named flag / piece bits;
  5. the sizes mccnn_conv_prepare reports are, byte for byte, those of the commit before the route record
     (tests/golden/conv_route_req.txt, written by tools/conv_route_check.hip built against that commit), computed by the same
     program built against this tree with the host's address and undefined-behaviour sanitizers (on a machine without a GPU).
Runs under a default environment (no MCCNN_ROW_KERNELS, no rows_* / unsorted_max_points key in MCCNN_DEBUG)."""
import itertools
import os
import re
import subprocess

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

COMBIN = (0, 1)
FIN = (1, 7, 8, 16, 128, 136, 248, 256, 264)
EDGES = (0, 1, 500000, 500001, 4194304, 16777216)
N_POINTS = (65535, 65536)
POINTERS = (0x1000, 0x1004, 0x1008, 0x1010)


def rows_of(e):
    return (0, 1, e // 16 - 1, e // 16, e // 16 + 1)


class _Rows:
    """What the rule below looks at of a feature tensor."""
    def __init__(self, pointer, n):
        self.pointer, self.shape = pointer, (n, 0)

    def data_ptr(self):
        return self.pointer


ROW_KERNELS, _DEBUG_IMPL, ROWS_MIN_DEGREE = True, 0, 16.0   # the defaults the rule below ran with


def _rows_shape_before(combin, fin, feats, rows, e, backward=False):
    # MCConvModule._rows_shape as it stood before it asked the library (body copied, comments dropped)
    if not (ROW_KERNELS and _DEBUG_IMPL == 0 and (not combin) and fin % 8 == 0 and e > 0 and rows > 0
            and (feats.data_ptr() & 15) == 0):
        return False
    if e <= 500000:
        return True
    if not backward:
        return not (fin <= 128 and feats.shape[0] >= 65536)
    return fin >= 256 and e / float(rows) >= ROWS_MIN_DEGREE


def _lattice():
    for combin, fin, e, n, backward in itertools.product(COMBIN, FIN, EDGES, N_POINTS, (0, 1)):
        for rows in rows_of(e):
            yield combin, fin, e, rows, n, backward


def test_query_is_the_rule_the_python_surface_stated():
    from mccnn_amd import _lib
    import mccnn_amd.MCConvModule as mc
    lib = _lib.load()
    mc.debug_conv_impl(0)
    count, taken = 0, 0
    for combin, fin, e, rows, n, backward in _lattice():
        for p in POINTERS:
            want = _rows_shape_before(combin, fin, _Rows(p, n), rows, e, bool(backward))
            got = lib.mccnn_conv_rows_shape(combin, fin, p, rows, n, e, backward)
            assert got == int(want), (combin, fin, e, rows, n, hex(p), backward, got, want)
            count, taken = count + 1, taken + got
    assert count == 2 * 9 * 6 * 5 * 2 * 4 * 2 and 0 < taken < count
    before = lib.mccnn_debug_launch_count()
    lib.mccnn_conv_rows_shape(0, 8, 0x1000, 10, 10, 100, 0)
    assert lib.mccnn_debug_launch_count() == before


def test_python_rule_asks_the_library():
    from mccnn_amd import _lib
    import mccnn_amd.MCConvModule as mc
    lib = _lib.load()
    mc.debug_conv_impl(0)
    rows_kernels = mc.ROW_KERNELS
    assert rows_kernels is True
    cases = list(_lattice())
    try:
        for n, fin in itertools.product(N_POINTS, FIN):
            base = torch.empty(n * fin + 4)
            assert base.data_ptr() % 16 == 0
            for t in (base[:n * fin].view(n, fin), base[1:1 + n * fin].view(n, fin)):
                assert t.data_ptr() % 16 == (0 if t.data_ptr() == base.data_ptr() else 4)
                mine = [c for c in cases if c[1] == fin and c[4] == n]
                for combin, _, e, rows, _, backward in mine:
                    want = bool(lib.mccnn_conv_rows_shape(combin, fin, t.data_ptr(), rows, n, e, backward))
                    assert mc._rows_shape(bool(combin), fin, t, rows, e, backward=bool(backward)) is want
                    if backward == 0:
                        assert mc._rows_shape(bool(combin), fin, t, rows, e) is want
                mc.ROW_KERNELS = False
                assert not any(mc._rows_shape(bool(c[0]), fin, t, c[3], c[2], backward=bool(c[5])) for c in mine)
                mc.ROW_KERNELS = True
                mc.debug_conv_impl(4)
                assert not any(mc._rows_shape(bool(c[0]), fin, t, c[3], c[2], backward=bool(c[5])) for c in mine)
                mc.debug_conv_impl(0)
            del base
        t = torch.empty((100, 8))
        assert mc._rows_shape(False, 8, t, 100, 1000) is True and mc._rows_shape(False, 8, t, 100, 1000, backward=True) is True
        for mask in (1, 2):   # bits 0-1 reach the library's rule, and the kept answers do not outlive the mask they were given under
            mc.debug_conv_impl(mask)
            assert mc._rows_shape(False, 8, t, 100, 1000) is False
            mc.debug_conv_impl(0)
            assert mc._rows_shape(False, 8, t, 100, 1000) is True
    finally:
        mc.ROW_KERNELS = rows_kernels
        mc.debug_conv_impl(0)


def test_unsorted_limit_is_the_librarys():
    from mccnn_amd import _lib
    import mccnn_amd.MCConvModule as mc
    assert mc.UNSORTED_MAX_POINTS == _lib.load().mccnn_conv_unsorted_max_points() == 32768
    assert not hasattr(mc, "ROWS_MIN_DEGREE")


def test_header_binding_and_library():
    import ctypes as C
    from mccnn_amd import _lib, build, native
    lib = _lib.load()
    assert lib.mccnn_abi_version() >= 31
    text = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    i, vp = C.c_int, C.c_void_p
    assert _lib.SIGNATURES["mccnn_conv_rows_shape"] == (i, [i, i, vp, i, i, i, i])
    assert _lib.SIGNATURES["mccnn_conv_unsorted_max_points"] == (i, [])
    assert {"mccnn_conv_rows_shape", "mccnn_conv_unsorted_max_points"} <= exported
    assert re.search(r"int\s+mccnn_conv_rows_shape\s*\(\s*int\s+combin\s*,\s*int\s+num_in_feats\s*,\s*const\s+void\s*\*\s*feats\s*,\s*int\s+rows\s*,"
                     r"\s*int\s+n_points\s*,\s*int\s+e\s*,\s*int\s+backward\s*\)\s*;", code)
    assert re.search(r"int\s+mccnn_conv_unsorted_max_points\s*\(\s*void\s*\)\s*;", code)
    assert "as the Python op surface chooses it" not in text
    defines = dict(re.findall(r"^#define\s+(MCCNN_(?:CONV|PIECE)_[A-Z_]+)\s+(\d+)\s*$", code, flags=re.M))
    assert defines == {"MCCNN_CONV_KEEP_STATE": "1", "MCCNN_CONV_DETERMINISTIC": "2", "MCCNN_CONV_READS_RECORDS": "4",
                       "MCCNN_PIECE_PLAN_FWD": "1", "MCCNN_PIECE_PLAN_TR": "2", "MCCNN_PIECE_TLIST": "4", "MCCNN_PIECE_RECORDS": "8"}
    assert (native.CONV_KEEP_STATE, native.CONV_DETERMINISTIC, native.CONV_READS_RECORDS) == (1, 2, 4)
    assert (native.NEED_PLAN_FWD, native.NEED_PLAN_TR, native.NEED_TLIST, native.NEED_RECORDS) == (1, 2, 4, 8)


def _code(path):
    src = open(path).read()
    if path.endswith(".py"):
        return re.sub(r'""".*?"""|#[^\n]*', "", src, flags=re.S)
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", src, flags=re.S)


def test_thresholds_live_in_one_source_file():
    """As code, 500000 and a parse of rows_min_degree / unsorted_max_points / rows_force stand in csrc/exec.hip alone (the lists of
    known MCCNN_DEBUG keys aside), the Python package compares nothing with 65536, and no bare flag literal is left in the
    executor or the extension."""
    edges, parses, points = set(), set(), set()
    for top in ("mccnn_amd", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if not f.endswith((".py", ".hip", ".h", ".cpp")):
                    continue
                src = _code(os.path.join(d, f))
                if re.search(r"\b500000\b", src):
                    edges.add(f)
                if re.search(r"debug(_int|_float)?\(\s*\"(rows_min_degree|unsorted_max_points|rows_force)\"", src):
                    parses.add(f)
                if f.endswith(".py") and re.search(r"\b65536\b", src):
                    points.add(f)
    assert edges == {"exec.hip"} and parses == {"exec.hip"} and not points
    for f in ("exec.hip", "torch_ext.cpp"):
        assert not re.search(r"flags\s*(&|\|=)\s*[124]\b", _code(os.path.join(ROOT, "mccnn_amd", "csrc", f))), f


def test_prepare_sizes_are_those_before_the_route_record(tmp_path):
    """tools/conv_route_check.hip: csrc/exec.hip with a main(), host code under -fsanitize=address,undefined. Its table over
    every kernel family, flags 0..7, both sides of every threshold and geometries with and without their pieces equals the one
    written at the commit before the route record, byte for byte, and the sanitizers report nothing."""
    from mccnn_amd import build
    lib = build.build()
    hipcc = build._hipcc()
    exe = str(tmp_path / "conv_route_check")
    # (the library the program links brings the HIP runtime along, and a sanitized process is not to open a GPU: where there
    # is one the program is built plain -- the comparison is the same, the sanitizers run wherever the suite runs without a GPU)
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g"] + sanitize + [
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mccnn_amd", "csrc"),
                           os.path.join(ROOT, "tools", "conv_route_check.hip"), "-L" + os.path.dirname(lib),
                           "-l:" + os.path.basename(lib), "-Wl,-rpath," + os.path.dirname(lib), "-o", exe], cwd=str(tmp_path))
    env = {k: v for k, v in os.environ.items() if k not in ("MCCNN_DEBUG", "MCCNN_ROW_KERNELS")}
    out = subprocess.run([exe], capture_output=True, env=env)
    assert out.returncode == 0 and out.stderr == b"", out.stderr.decode()[-2000:]
    golden = open(os.path.join(HERE, "golden", "conv_route_req.txt"), "rb").read()
    assert len(golden) > 100000 and out.stdout == golden
    routes = subprocess.run([exe, "--routes"], capture_output=True, env=env, check=True).stdout.decode()
    seen = set(re.findall(r"\[rows (\d\d) unsorted (\d) family (\d) f1 (\d)", routes))
    assert {r[0] for r in seen} == {"00", "10", "11"} and {r[1] for r in seen} == {"0", "1"} and {r[2] for r in seen} == {"0", "1", "2"}
    assert set(re.findall(r"tlist (\d)\]", routes)) == {"0", "1", "2"}
