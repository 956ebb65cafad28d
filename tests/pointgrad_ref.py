"""Float64 torch restatement of the forward of spatial_conv, compute_pdf and the box / radius dependence, for the tests of the
gradients with respect to positions. The integer structure (CSR start indices, packed neighbour list, sort and Poisson
indices) is an INPUT: every discrete decision of the forward pass is held fixed, and torch autograd differentiates the rest.

Formulas (README, "Gradients with respect to point positions"):
  R_b      = radius * maxExtent_b (scaleInv; the longest axis, the lowest one on a tie) or radius
  delta    = (p_j - c_i) / R_b
  out[i]  += f[j, fin(nu)] * a_nu(delta) / (pdf_t * K_i)        a = the kernel MLP, flat layouts w1[nu*3+d], w2/w3[q*64+o*8+k]
  pdf_t    = (1/k_i) sum_{t' in row i} prod_d (0.39894228 / h) exp(-((p_j' - p_j)_d / (R_b h))^2 / 2)
"""
import numpy as np
import torch

MLP = 8
C_PHI = 0.39894228   # the KDE's constant as the kernels use it


def t64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def radius_per_batch(mn, mx, radius, scaleInv):
    """[B] radii; the axis choice is held fixed (argmax = first maximum, as max(max(x, y), z) picks on a tie)."""
    if not scaleInv:
        return torch.full((mn.shape[0],), float(radius), dtype=torch.float64)
    ext = mx - mn
    axis = ext.detach().argmax(dim=1, keepdim=True)
    return float(radius) * ext.gather(1, axis).squeeze(1)


FLT_MAX = float(np.finfo(np.float32).max)


def box_of(pts, bids, B, scaleInv):
    """compute_aabb: per-batch min / max (scaleInv) or the whole-batch box in every row; ties share the gradient. A batch
    without points gets the kernels' empty box (FLT_MAX, -FLT_MAX), a constant."""
    b = torch.as_tensor(np.asarray(bids).reshape(-1)).long()
    if not scaleInv:
        mn, mx = pts.amin(0), pts.amax(0)
        return mn.expand(B, 3), mx.expand(B, 3)
    full = lambda v: torch.full((3,), v, dtype=pts.dtype)
    mns = [pts[b == k].amin(0) if bool((b == k).any()) else full(FLT_MAX) for k in range(B)]
    mxs = [pts[b == k].amax(0) if bool((b == k).any()) else full(-FLT_MAX) for k in range(B)]
    return torch.stack(mns), torch.stack(mxs)


def _rows(start, e):
    start = np.asarray(start).reshape(-1).astype(np.int64)
    end = np.append(start[1:], e)
    return start, end


def spatial_conv(pts, feats, bids, pdfs, smp, start, packed, mn, mx, w1, b1, w2, b2, w3, b3, fout, combin, B, radius,
                 scaleInv, avg):
    """pts [N,3], feats [N,Fin], pdfs [E] or [E,1], smp [M,3], mn / mx [B,3], the six MLP tensors (any shape, flat layouts
    as above): float64 tensors (requires_grad as wanted). bids, start [M], packed [E,2]: integer arrays. -> out [M, outF]"""
    packed = np.asarray(packed).reshape(-1, 2).astype(np.int64)
    e = packed.shape[0]
    m = smp.shape[0]
    fin = feats.shape[1]
    neurons = fin * fout if combin else fin
    nb = (neurons + MLP - 1) // MLP
    outF = fout if combin else fin
    j = torch.as_tensor(packed[:, 0])
    c = torch.as_tensor(packed[:, 1])
    b = torch.as_tensor(np.asarray(bids).reshape(-1).astype(np.int64))[j]
    R = radius_per_batch(mn, mx, radius, scaleInv)[b]
    delta = (pts[j] - smp[c]) / R[:, None]
    W1 = w1.reshape(-1).view(nb * MLP, 3)
    W2 = w2.reshape(-1).view(nb, MLP, MLP)
    W3 = w3.reshape(-1).view(nb, MLP, MLP)
    h1 = torch.relu(delta @ W1.t() + b1.reshape(-1)).view(e, nb, MLP)
    h2 = torch.relu(torch.einsum("eqk,qok->eqo", h1, W2) + b2.reshape(nb, MLP))
    a = (torch.einsum("eqk,qok->eqo", h2, W3) + b3.reshape(nb, MLP)).reshape(e, nb * MLP)[:, :neurons]
    nu = np.arange(neurons)
    fi = nu % fin if combin else nu
    fo = nu // fin if combin else nu
    s0, s1 = _rows(start, e)
    K = torch.as_tensor((s1 - s0).astype(np.float64)) if avg else torch.ones(m, dtype=torch.float64)
    contrib = feats[j][:, torch.as_tensor(fi)] * a / (pdfs.reshape(-1) * K[c])[:, None]
    S = torch.zeros((neurons, outF), dtype=torch.float64)
    S[torch.as_tensor(nu), torch.as_tensor(fo)] = 1.0
    return torch.zeros((m, outF), dtype=torch.float64).index_add(0, c, contrib @ S)


def compute_pdf(pts, bids, mn, mx, start, packed, window, radius, scaleInv, pair_budget=None):
    """-> pdfs [E] (float64) of the sorted points `pts` over the fixed neighbour list. pair_budget: evaluate in groups of
    consecutive slots of at most that many (slot, row member) pairs (a longer row is split between groups); same values."""
    if pair_budget is not None:
        j, Re, first, k = _pdf_setup(bids, mn, mx, start, packed, radius, scaleInv)
        X = pts[torch.as_tensor(j)]
        parts = [_pdf_slots(X, Re, first, k, a, b, window) for a, b in _slot_groups(k, pair_budget)]
        return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float64)
    packed = np.asarray(packed).reshape(-1, 2).astype(np.int64)
    e = packed.shape[0]
    s0, s1 = _rows(start, e)
    row = packed[:, 1]
    k = (s1 - s0)[row]
    t = np.repeat(np.arange(e), k)
    first = np.repeat(s0[row], k)
    within = np.arange(t.shape[0]) - np.repeat(np.cumsum(k) - k, k)
    tp = first + within
    j, jp = torch.as_tensor(packed[t, 0]), torch.as_tensor(packed[tp, 0])
    b = torch.as_tensor(np.asarray(bids).reshape(-1).astype(np.int64))[j]
    R = radius_per_batch(mn, mx, radius, scaleInv)[b]
    x = (pts[jp] - pts[j]) / (R * window)[:, None]
    g = torch.prod((C_PHI / window) * torch.exp(-0.5 * x * x), dim=1)
    tot = torch.zeros(e, dtype=torch.float64).index_add(0, torch.as_tensor(t), g)
    return tot / torch.as_tensor(k.astype(np.float64))


# ---------------------------------------------------------------------------------------------- per-edge forms
#: Ambiguity threshold of a ReLU: the kernels' float32 pre-activation takes ~11 roundings (delta's quotient, the fma chain,
#: the bias), so it lies within 11 * 2^-24 S < 2^-20.5 S of the exact value (S: the chain's magnitude, see conv_preacts).
#: 2^-18 is 8x over that; where |pre| <= TAU S the sign the kernels see is not decided by the reference.
TAU = 2.0 ** -18


def _pdf_setup(bids, mn, mx, start, packed, radius, scaleInv):
    """Per slot t of the KDE: its point j, its radius R (a tensor: differentiable through mn / mx), the first slot and the
    length of its row."""
    packed = np.asarray(packed).reshape(-1, 2).astype(np.int64)
    e = packed.shape[0]
    s0, s1 = _rows(start, e)
    row, j = packed[:, 1], packed[:, 0]
    b = np.asarray(bids).reshape(-1).astype(np.int64)[j]
    Re = radius_per_batch(mn, mx, radius, scaleInv)[torch.as_tensor(b)]
    return j, Re, s0[row], (s1 - s0)[row]


def _slot_groups(k, budget):
    """[a, b) ranges of consecutive slots whose pair counts (each slot pairs with its whole row) sum to <= budget; a slot
    whose row alone exceeds it forms a group of one."""
    cum = np.concatenate([[0], np.cumsum(np.asarray(k, np.int64))])
    out, a = [], 0
    while a < len(k):
        b = max(int(np.searchsorted(cum, cum[a] + budget, side="right")) - 1, a + 1)
        out.append((a, b))
        a = b
    return out


def _pdf_slots(X, Re, first, k, a, b, window):
    """pdf_t of the slots [a, b) from the per-slot positions X [E,3] and radii Re [E] (the pairs summed in row order)."""
    kk = k[a:b]
    t = np.repeat(np.arange(a, b), kk)
    tp = np.repeat(first[a:b], kk) + (np.arange(t.shape[0]) - np.repeat(np.cumsum(kk) - kk, kk))
    tt = torch.as_tensor(t)
    x = (X[torch.as_tensor(tp)] - X[tt]) / (Re[tt] * window)[:, None]
    g = torch.prod((C_PHI / window) * torch.exp(-0.5 * x * x), dim=1)
    tot = torch.zeros(b - a, dtype=torch.float64).index_add(0, torch.as_tensor(t - a), g)
    return tot / torch.as_tensor(kk.astype(np.float64))


def pdf_edge_grads(pts, bids, mn, mx, start, packed, window, radius, scaleInv, gpdf, pair_budget=1 << 20):
    """Per-slot gradients of L = sum_t gpdf[t] pdf_t, in the form the kernel stores them: dp [E,3] with respect to slot t's
    own copy of its point (its terms as t and as a row member t') and dR [E] with respect to slot t's own radius. Evaluated
    in slot groups under `pair_budget`. Inputs are arrays. -> float64 numpy (dp, dR)."""
    e = np.asarray(packed).reshape(-1, 2).shape[0]
    if e == 0:
        return np.zeros((0, 3)), np.zeros(0)
    j, Rb, first, k = _pdf_setup(bids, t64(mn), t64(mx), start, packed, radius, scaleInv)
    X = t64(pts)[torch.as_tensor(j)].requires_grad_(True)
    Re = Rb.detach().clone().requires_grad_(True)
    gp = t64(gpdf).reshape(-1)
    for a, b in _slot_groups(k, pair_budget):
        (_pdf_slots(X, Re, first, k, a, b, window) * gp[a:b]).sum().backward()
    return X.grad.numpy(), Re.grad.numpy()


def _mlp64(w):
    nb = np.asarray(w["b1"]).size // MLP
    T = lambda a: t64(a).reshape(-1)
    return (nb, T(w["w1"]).view(nb * MLP, 3), T(w["b1"]), T(w["w2"]).view(nb, MLP, MLP), T(w["b2"]).view(nb, MLP),
            T(w["w3"]).view(nb, MLP, MLP), T(w["b3"]).view(nb, MLP))


def _edge_delta(pts, smp, bids, packed, mn, mx, radius, scaleInv, sel):
    j, c = packed[sel, 0], packed[sel, 1]
    b = np.asarray(bids).reshape(-1).astype(np.int64)[j]
    R = radius_per_batch(t64(mn), t64(mx), radius, scaleInv)[torch.as_tensor(b)]
    return j, c, R


def conv_preacts(pts, smp, bids, packed, mn, mx, w, radius, scaleInv, sel):
    """float64 pre-activations of the kernel MLP's two ReLU layers on the edges `sel` and their magnitudes:
    S1 = sum_d |delta_d| |w1| + |b1|,  S2 = sum_k (S1_k + h1_k) |w2| + |b2|  (layer 1's bound carried into layer 2).
    -> (pre1, S1, pre2, S2), each [len(sel), nb * 8]."""
    packed = np.asarray(packed).reshape(-1, 2).astype(np.int64)
    nb, W1, b1, W2, b2, _, _ = _mlp64(w)
    j, c, R = _edge_delta(pts, smp, bids, packed, mn, mx, radius, scaleInv, sel)
    delta = (t64(pts)[torch.as_tensor(j)] - t64(smp)[torch.as_tensor(c)]) / R[:, None]
    pre1 = delta @ W1.t() + b1
    S1 = delta.abs() @ W1.abs().t() + b1.abs()
    n = len(sel)
    h1 = torch.relu(pre1).view(n, nb, MLP)
    pre2 = torch.einsum("eqk,qok->eqo", h1, W2) + b2
    S2 = torch.einsum("eqk,qok->eqo", S1.view(n, nb, MLP) + h1, W2.abs()) + b2.abs()
    return pre1, S1, pre2.reshape(n, -1), S2.reshape(n, -1)


def conv_ambiguity(pts, smp, bids, packed, mn, mx, w, radius, scaleInv, tau=TAU, chunk=8192):
    """The (edge, layer, neuron) triples whose float64 pre-activation satisfies |pre| <= tau * S (conv_preacts): there the
    kernels' float32 ReLU' = 1[pre >= 0] may differ from the reference's. Layer 3 and the KDE have no ReLU.
    -> int64 [A, 3], sorted by edge."""
    packed = np.asarray(packed).reshape(-1, 2).astype(np.int64)
    out = []
    for a in range(0, packed.shape[0], chunk):
        sel = np.arange(a, min(a + chunk, packed.shape[0]))
        pre1, S1, pre2, S2 = conv_preacts(pts, smp, bids, packed, mn, mx, w, radius, scaleInv, sel)
        for layer, pre, S in ((1, pre1, S1), (2, pre2, S2)):
            e_, nu = np.nonzero((pre.abs() <= tau * S).numpy())
            out.append(np.stack([sel[e_], np.full(len(e_), layer), nu], 1))
    a = np.concatenate(out) if out else np.zeros((0, 3), np.int64)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))].astype(np.int64)


def conv_edge_grads(pts, feats, bids, pdfs, smp, start, packed, mn, mx, w, og, fout, combin, radius, scaleInv, avg,
                    edges=None, force=None, chunk=4096):
    """Per-edge gradients of L = sum(spatial_conv(...) * og), made leaves of the gathered pts[j] and smp[c] ([n,3]), of the
    edge's PDF and of the edge's own radius R: dp [n,3], dc [n,3], dpdf [n], dR [n], and the edge's delta [n,3], for the
    edges `edges` (default all; repeats allowed). Inputs are arrays (bf16 features already rounded); w: the six MLP arrays.
    ReLU' is 1[pre >= 0] (the kernels' convention at 0); force = {layer (1 | 2): (rows, neurons, values)} sets it to
    `values` for those (position in `edges`, neuron) pairs instead. -> dict of float64 numpy arrays."""
    packed = np.asarray(packed).reshape(-1, 2).astype(np.int64)
    e = packed.shape[0]
    sel_all = np.arange(e) if edges is None else np.asarray(edges, np.int64).reshape(-1)
    s0, s1 = _rows(start, e)
    klen = (s1 - s0).astype(np.float64)
    F64, O64 = t64(feats), t64(og)
    res = {k: [] for k in ("dp", "dc", "dpdf", "dR", "delta")}
    for a in range(0, len(sel_all), chunk):
        sel = sel_all[a:a + chunk]
        n = len(sel)
        j, c, Rb = _edge_delta(pts, smp, bids, packed, mn, mx, radius, scaleInv, sel)
        P = t64(pts)[torch.as_tensor(j)].requires_grad_(True)
        Cc = t64(smp)[torch.as_tensor(c)].requires_grad_(True)
        pd = t64(pdfs).reshape(-1)[torch.as_tensor(sel)].requires_grad_(True)
        R = Rb.detach().clone().requires_grad_(True)
        K = torch.as_tensor(klen[c]) if avg else torch.ones(n, dtype=torch.float64)
        terms, delta = conv_edge_terms(P, Cc, pd, R, F64[torch.as_tensor(j)], O64[torch.as_tensor(c)], K, w, fout, combin,
                                       force, a)
        loss = terms.sum()
        loss.backward()
        for k, v in (("dp", P.grad), ("dc", Cc.grad), ("dpdf", pd.grad), ("dR", R.grad), ("delta", delta.detach())):
            res[k].append(v.numpy())
    return {k: (np.concatenate(v) if v else np.zeros((0,) + ((3,) if k in ("dp", "dc", "delta") else ())))
            for k, v in res.items()}


def conv_edge_terms(P, Cc, pd, R, Fj, Oc, K, w, fout, combin, force=None, a=0):
    """The per-edge form of L = sum(spatial_conv(...) * og): edge e's term sum_nu Fj[e, fin(nu)] a_nu(delta_e)
    Oc[e, fo(nu)] / (pd_e K_e) with delta_e = (P_e - Cc_e) / R_e. P, Cc [n,3], pd, R, K [n], Fj [n,Fin] (the neighbour's
    features), Oc [n,outF] (the centre's out-gradient): float64 tensors; w: the six MLP arrays; force, a: see
    conv_edge_grads (a = the position of row 0 in `edges`). -> (terms [n], delta [n,3])"""
    n, fin = Fj.shape
    neurons = fin * fout if combin else fin
    nb, W1, b1, W2, b2, W3, b3 = _mlp64(w)
    nu = np.arange(neurons)
    fi = torch.as_tensor(nu % fin if combin else nu)
    fo = torch.as_tensor(nu // fin if combin else nu)
    delta = (P - Cc) / R[:, None]
    pre1 = delta @ W1.t() + b1
    h1 = (pre1 * _mask(pre1, force, 1, a, n)).view(n, nb, MLP)
    pre2 = (torch.einsum("eqk,qok->eqo", h1, W2) + b2).reshape(n, nb * MLP)
    h2 = (pre2 * _mask(pre2, force, 2, a, n)).view(n, nb, MLP)
    act = (torch.einsum("eqk,qok->eqo", h2, W3) + b3).reshape(n, nb * MLP)[:, :neurons]
    return (Fj[:, fi] * act * Oc[:, fo]).sum(1) / (pd * K), delta


def _mask(pre, force, layer, a, n):
    m = (pre.detach() >= 0).to(torch.float64)
    if force and layer in force:
        rows, nus, vals = (np.asarray(x) for x in force[layer])
        keep = (rows >= a) & (rows < a + n)
        if keep.any():
            m[torch.as_tensor(rows[keep] - a), torch.as_tensor(nus[keep])] = torch.as_tensor(vals[keep], dtype=torch.float64)
    return m
