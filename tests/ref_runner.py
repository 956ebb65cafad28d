"""Runs named cases of tests/ref_cases.py through the REFERENCE's own kernels (oracle/ref.py over
oracle/_ref/libmccnn_ref.so) on the GPU and writes one <case>.npz of its outputs per case.

    python tests/ref_runner.py --out DIR [case ...]     every case (or the named ones) -> DIR/<case>.npz
    python tests/ref_runner.py --golden [--out DIR]     the smallest cases -> tests/golden/ref_<case>.npz (fixtures of
                                                        tests/test_oracle_pinned_cpu.py; recorded results only)

It is a script, not a test module: the reference was written for another vendor's GPU, so it runs in a process of its
own (tests/test_gpu_reference.py starts it once, as a child) and a fault in it takes nothing else along. Each op is fed
the ORACLE's outputs of the preceding ops (see tests/ref_cases.py). One line per case goes to stdout before the case
starts, so the log names the case a fault belongs to.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--golden", action="store_true")
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args(argv)
    from tests import ref_cases as rc
    from oracle.oracle import Oracle
    from oracle.ref import Reference
    names = a.cases or (rc.GOLDEN_CASES if a.golden else [c["name"] for c in rc.CASES])
    out_dir = a.out or (os.path.join(ROOT, "tests", "golden") if a.golden else None)
    if out_dir is None:
        ap.error("--out is required without --golden")
    os.makedirs(out_dir, exist_ok=True)
    orc, ref = Oracle(), Reference()
    for name in names:
        case = rc.CASE_BY_NAME[name]
        print("case %s ..." % name, flush=True)
        t0 = time.time()
        inp = rc.make_inputs(case)
        o = rc.run_ops(orc, case, inp)
        t1 = time.time()
        r = rc.public(rc.run_ops(ref, case, inp, src=o))
        path = os.path.join(out_dir, ("ref_%s.npz" if a.golden else "%s.npz") % name)
        np.savez_compressed(path, **r)
        print("case %s done: oracle %.1f s, reference %.1f s, %d bytes" % (name, t1 - t0, time.time() - t1,
                                                                          os.path.getsize(path)), flush=True)
    if not a.golden:   # the parent takes this file, not the exit status alone, as "every case was written"
        with open(os.path.join(out_dir, "runner_done.txt"), "w") as f:
            f.write("\n".join(names) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
