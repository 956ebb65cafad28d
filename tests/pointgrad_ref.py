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


def box_of(pts, bids, B, scaleInv):
    """compute_aabb: per-batch min / max (scaleInv) or the whole-batch box in every row; ties share the gradient."""
    b = torch.as_tensor(np.asarray(bids).reshape(-1)).long()
    if not scaleInv:
        mn, mx = pts.amin(0), pts.amax(0)
        return mn.expand(B, 3), mx.expand(B, 3)
    mns = [pts[b == k].amin(0) for k in range(B)]
    mxs = [pts[b == k].amax(0) for k in range(B)]
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


def compute_pdf(pts, bids, mn, mx, start, packed, window, radius, scaleInv):
    """-> pdfs [E] (float64) of the sorted points `pts` over the fixed neighbour list."""
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
