"""find_neighbors(maxNeighbors=K) on the 100k room: ms per call (count + scan + fill, HIP events, the op with its edge-count
read-back) and the resulting E, for K = 0 (no cap) and every cap on the command line (default 32 64). --seed S: every cap is
timed a second time with find_neighbors(sampleSeed=S), the stratified sample beside the canonical ranks (same count pass and
scan: the difference of the two lines is the difference of the fill passes)."""
import sys, os, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mccnn_amd import MCConvModule as M
from mccnn_amd.workloads import make_room
argv, seed = sys.argv[1:], None
if "--seed" in argv:
    seed = int(argv[argv.index("--seed") + 1])
    del argv[argv.index("--seed"):argv.index("--seed") + 2]
caps = [0] + [int(a) for a in argv] if argv else [0, 32, 64]
runs = [(K, {"maxNeighbors": K} if K else {}) for K in caps]
if seed is not None:
    runs += [(K, {"maxNeighbors": K, "sampleSeed": seed}) for K in caps if K]
    runs.sort(key=lambda r: caps.index(r[0]))   # (stable: canonical, then sampled, per cap)
P = torch.from_numpy(make_room(100000, 20180601)).cuda()
Bi = torch.zeros((P.shape[0], 1), dtype=torch.int32, device=P.device)
mn, mx = M.compute_aabb(P, Bi, 1, False)
sP, sB, cells, idx, inv = M.build_grid(P, Bi, mn, mx, 1, 0.1, False)
for K, kw in runs:
    for _ in range(10):
        st, pk = M.find_neighbors(P, Bi, sP, cells, mn, mx, 0.1, 1, False, **kw)
    torch.cuda.synchronize()
    best = 1e9
    for rep in range(5):   # best of five runs of 50 calls: the spread between runs is printed too
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            st, pk = M.find_neighbors(P, Bi, sP, cells, mn, mx, 0.1, 1, False, **kw)
        e1.record(); torch.cuda.synchronize()
        t = e0.elapsed_time(e1) / 50
        best = min(best, t)
        worst = t if rep == 0 else max(worst, t)
    k = torch.diff(torch.cat([st.view(-1).long(), torch.tensor([pk.shape[0]], device=st.device)]))
    print("maxNeighbors %-4d %-14s find_neighbors ms %.4f (worst of 5: %.4f)  E %d  max row %d"
          % (K, "sampleSeed %d" % seed if "sampleSeed" in kw else "", best, worst, pk.shape[0], int(k.max())))
