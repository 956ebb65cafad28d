"""The expected output of find_neighbors(maxNeighbors=K, sampleSeed=s): the uncapped list (the oracle's), thinned row by row
in NumPy. Geometries and uncapped() are those of tests/neighbor_cap_ref.py.

Rule (0 < K < k, seed s in [0, 2^32), i = the row's index in the list; exact integers):
    lo_t  = floor(t * k / K), t = 0 .. K          stratum t = canonical ranks [lo_t, lo_{t+1}), len_t >= 1
    mix(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16      (uint32)
    h     = mix(mix(s + 0x9E3779B9 * (i + 1)) + t)                                           (uint32)
    off_t = (h * len_t) >> 32                                                                (a 64-bit product)
slot t holds the hit at canonical rank lo_t + off_t. Rows of k <= K hits are unchanged; startIndexs is the exclusive prefix
sum of min(k, K), as under the canonical cap (which is "off_t = 0")."""
import numpy as np

from tests.neighbor_cap_ref import GEOMETRIES, cap_list, row_lengths, uncapped, window_sizes  # noqa: F401 (re-exported)

M32 = 0xFFFFFFFF


def mix(x):
    """The murmur3 finaliser on uint32; x an int or an integer array, result uint64 array / int below 2^32."""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def strata(k, K):
    """lo_t, t = 0 .. K, of a row of k > K hits: int64 [K + 1]. Python integers where t * k could pass 2^63."""
    k, K = int(k), int(K)
    assert 0 < K < k
    if k * K < (1 << 62):
        return (np.arange(K + 1, dtype=np.int64) * k) // K
    return np.asarray([(t * k) // K for t in range(K + 1)], np.int64)


def offsets(i, k, K, seed, zero=False):
    """off_t, t = 0 .. K-1, of row i: int64 [K]. zero=True: the canonical cap's choice."""
    lo = strata(k, K)
    if zero:
        return np.zeros(int(K), np.int64)
    a = int(mix((int(seed) + 0x9E3779B9 * (int(i) + 1)) & M32))
    h = mix((a + np.arange(int(K), dtype=np.uint64)) & np.uint64(M32))
    return ((h * np.diff(lo).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)   # h < 2^32, len_t < 2^31: no overflow


def sample_ranks(i, k, K, seed, zero=False):
    """Canonical ranks row i of k hits keeps under cap K and the seed, ascending: int64 [min(k, K)]."""
    k, K = int(k), int(K)
    if k <= K:
        return np.arange(k, dtype=np.int64)
    return strata(k, K)[:-1] + offsets(i, k, K, seed, zero)


def sample_slot(r, i, k, K, seed):
    """Per-hit form (the fill pass): slot of the hit at rank r of row i, or -1 when the sample drops it (Python integers)."""
    r, i, k, K = int(r), int(i), int(k), int(K)
    if k <= K:
        return r
    t = ((r + 1) * K - 1) // k
    lo, hi = (t * k) // K, ((t + 1) * k) // K
    a = int(mix((int(seed) + 0x9E3779B9 * (i + 1)) & M32))
    off = (int(mix((a + t) & M32)) * (hi - lo)) >> 32
    return t if r == lo + off else -1


def sample_list(start, packed, K, seed, zero=False):
    """(startIndexs [M,1] i32, packedNeighs [E,2] i32) of an uncapped CSR list -> the same pair under cap K > 0 and the seed."""
    start = np.asarray(start)
    packed = np.asarray(packed).reshape(-1, 2)
    K = int(K)
    assert K > 0 and 0 <= int(seed) <= M32
    st = start.reshape(-1).astype(np.int64)
    k = row_lengths(st, len(packed))
    kept = np.minimum(k, K)
    new_start = np.concatenate([[0], np.cumsum(kept)[:-1]]).astype(np.int64) if len(k) else np.zeros(0, np.int64)
    src = [st[i] + sample_ranks(i, k[i], K, seed, zero) for i in range(len(k))]
    src = np.concatenate(src).astype(np.int64) if src else np.zeros(0, np.int64)
    return new_start.astype(np.int32).reshape(-1, 1), np.ascontiguousarray(packed[src]).astype(np.int32)
