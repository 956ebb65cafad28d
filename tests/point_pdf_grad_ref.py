"""TEST INFRASTRUCTURE for the position gradients of pdfMode='point': the definition of compute_pdf_points / expand_pdf
(tests/point_pdf_ref.py: density_ref / expand_ref) restated in torch float64 over GIVEN integer rows, so that torch autograd
differentiates it with respect to the points and, through R_b = tests/pointgrad_ref.radius_per_batch, the box. Every discrete
decision (the rows, their lengths, the longest box axis) is an input and held fixed. Nothing here assumes that the rows are
symmetric. closed_form() is the kernels' formula in NumPy float64, for the CPU test that ties the two together.
Never imported by the product package."""
import numpy as np
import torch

from tests import pointgrad_ref as pg

C_PHI = pg.C_PHI


def density(pts, bids, mn, mx, packed, window, radius, scaleInv):
    """pts [N,3], mn / mx [B,3]: float64 tensors (requires_grad as wanted); bids [N]: integers; packed [E,2]: the rows of the
    search with the sorted points as their own centres, (l, j) = (neighbour, centre). -> density [N] float64:
    density[j] = sum over l in N(j) of prod_a (1/h) 0.39894228 exp(-0.5 ((p_l,a - p_j,a) / (R_b h))^2); 0 for an empty row."""
    packed = np.asarray(packed).reshape(-1, 2).astype(np.int64)
    n = pts.shape[0]
    l, j = torch.as_tensor(packed[:, 0]), torch.as_tensor(packed[:, 1])
    b = torch.as_tensor(np.asarray(bids).reshape(-1).astype(np.int64))[j]
    R = pg.radius_per_batch(mn, mx, radius, scaleInv)[b]
    h = float(np.float32(window))
    x = (pts[l] - pts[j]) / (R * h)[:, None]
    g = torch.prod((1.0 / h) * C_PHI * torch.exp(-0.5 * x * x), dim=1)
    return torch.zeros(n, dtype=torch.float64).index_add(0, j, g)


def expand(dens, start, packed):
    """dens [N] or [N,1] float64 tensor; start [M], packed [E,2] = (point j, centre i): integers. -> pdfs [E] float64:
    density[j] / len_i."""
    packed = np.asarray(packed).reshape(-1, 2).astype(np.int64)
    st = np.asarray(start).reshape(-1).astype(np.int64)
    k = np.diff(np.append(st, packed.shape[0])).astype(np.float64)
    return dens.reshape(-1)[torch.as_tensor(packed[:, 0])] / torch.as_tensor(k[packed[:, 1]])


def sweep_grads(pts, bids, mn, mx, packed, window, radius, scaleInv, gd):
    """Autograd of L = sum_j gd[j] density[j] -> (dpts [N,3], box [2B,3] = (dL/dmn; dL/dmx), or None without scaleInv), float64
    NumPy arrays. Inputs are arrays."""
    P = pg.t64(pts).requires_grad_(True)
    MN, MX = pg.t64(mn).requires_grad_(bool(scaleInv)), pg.t64(mx).requires_grad_(bool(scaleInv))
    d = density(P, bids, MN, MX, packed, window, radius, scaleInv)
    (d * pg.t64(gd).reshape(-1)).sum().backward()
    dp = P.grad.numpy() if P.grad is not None else np.zeros(tuple(P.shape))
    if not scaleInv:
        return dp, None
    zero = lambda t: t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))
    return dp, np.concatenate([zero(MN), zero(MX)])


def expand_grads(n, start, packed, g):
    """Autograd of L = sum_e g[e] pdfs[e] with respect to the density -> gd [N] float64 NumPy."""
    d = torch.ones(n, dtype=torch.float64, requires_grad=True)
    if np.asarray(packed).size == 0:
        return np.zeros(n)
    (expand(d, start, packed) * pg.t64(g).reshape(-1)).sum().backward()
    return d.grad.numpy()


def closed_form(pts, bids, mn, mx, packed, window, radius, scaleInv, gd):
    """The kernels' closed form in NumPy float64 over the rows (l, j):
        dpts[j] = -s_b^2 norm sum_{l in N(j)} (gd[j] + gd[l]) w_jl (p_j - p_l)
        dR[b]   = sum_{j in b} gd[j] norm (s_b^2 / R_b) sum_{l in N(j)} w_jl d2_jl
    -> (dpts [N,3], dR [B]); dR -> the box through box_from_dR. It IS the gradient only where the rows are symmetric."""
    packed = np.asarray(packed).reshape(-1, 2).astype(np.int64)
    P = np.asarray(pts, np.float64)
    n, B = len(P), len(np.asarray(mn))
    l, j = packed[:, 0], packed[:, 1]
    b = np.asarray(bids).reshape(-1).astype(np.int64)
    Rb = pg.radius_per_batch(pg.t64(mn), pg.t64(mx), radius, scaleInv).numpy()
    h = float(np.float32(window))
    norm = ((1.0 / h) * C_PHI) ** 3
    gd = np.asarray(gd, np.float64).reshape(-1)
    R = Rb[b[j]]
    s2 = 1.0 / (R * h) ** 2
    D = P[j] - P[l]
    d2 = (D * D).sum(1)
    w = np.exp(-0.5 * s2 * d2)
    c = -s2 * norm * (gd[j] + gd[l]) * w
    dpts = np.stack([np.bincount(j, weights=c * D[:, a], minlength=n) for a in range(3)], 1) if len(j) else np.zeros((n, 3))
    per_point = np.bincount(j, weights=gd[j] * norm * (s2 / R) * w * d2, minlength=n) if len(j) else np.zeros(n)
    dR = np.bincount(b, weights=per_point, minlength=B)
    return dpts, dR


def box_from_dR(mn, mx, dR, radius):
    """dL/dR_b -> [2B,3] = (dL/dmn; dL/dmx) through R_b = radius * (the longest axis, the lowest one on a tie)."""
    ext = np.asarray(mx, np.float64) - np.asarray(mn, np.float64)
    axis = ext.argmax(axis=1)
    g = np.zeros_like(ext)
    g[np.arange(len(ext)), axis] = np.asarray(dR, np.float64) * float(radius)
    return np.concatenate([-g, g])
