"""The numpy restatement of cae_case_neighbours (include/cae_hip.h).

Operands: queries (n_q, D) and references (n_r, D), fp32 rows.  A row is valid when all its D values are finite.  The
distance is the difference form d2(i, j) = S_d (double(q_d) - double(r_d))^2: fp64 differences, squared and summed (numpy's
pairwise sum here; the kernel folds d ascending with fused multiply-adds - on values where every operation is exact the two
agree bit for bit, elsewhere within (2 D + 8) 2^-53 relative).  Candidates of a query are the valid references other than
its own row (global index self_offset + i, where self_offset >= 0), ordered by (d2, global index ref_base + j) ascending
(np.lexsort).  Per query: dist2[K] ascending, index[K] global, unused slots +inf / -1, count in 0 .. K; an invalid query has
count -1, every dist2 +inf and every index -1.  merge: the lists of earlier calls over references with other global indices
join the candidates, and the K smallest of the union are kept."""
import numpy as np


def valid_rows(x):
    x = np.asarray(x)
    return np.isfinite(x.reshape(x.shape[0], -1)).all(axis=1) if x.shape[0] else np.zeros(0, dtype=bool)


def dist2(q, r, rows=64):
    """(n_q, n_r) float64: the difference form; pairs with an invalid row hold whatever the arithmetic gives"""
    q = np.asarray(q, dtype=np.float32).reshape(len(q), -1).astype(np.float64)
    r = np.asarray(r, dtype=np.float32).reshape(len(r), -1).astype(np.float64)
    out = np.empty((q.shape[0], r.shape[0]), dtype=np.float64)
    with np.errstate(all="ignore"):
        for i0 in range(0, q.shape[0], rows):
            diff = q[i0:i0 + rows, None, :] - r[None, :, :]
            out[i0:i0 + rows] = (diff * diff).sum(axis=-1)
    return out


def neighbours(q, r, k, ref_base=0, self_offset=None, merge_into=None, d2=None):
    """(dist2 (n_q, k) float64, index (n_q, k) int32, count (n_q,) int32); d2: the distances where the caller has them"""
    q = np.asarray(q, dtype=np.float32).reshape(len(q), -1)
    r = np.asarray(r, dtype=np.float32).reshape(len(r), -1)
    (n_q, n_r) = (q.shape[0], r.shape[0])
    d2 = dist2(q, r) if d2 is None else np.asarray(d2, dtype=np.float64)
    (q_ok, r_ok) = (valid_rows(q), valid_rows(r))
    out_d = np.full((n_q, k), np.inf, dtype=np.float64)
    out_i = np.full((n_q, k), -1, dtype=np.int32)
    count = np.zeros(n_q, dtype=np.int32)
    gidx = ref_base + np.arange(n_r, dtype=np.int64)
    for i in range(n_q):
        if not q_ok[i]:
            count[i] = -1
            continue
        keep = r_ok.copy()
        if self_offset is not None and self_offset >= 0:
            keep &= gidx != self_offset + i
        (cd, ci) = (d2[i, keep], gidx[keep])
        if merge_into is not None:
            (md, mi, _) = merge_into
            held = np.asarray(mi[i]) >= 0
            cd = np.concatenate([np.asarray(md[i], dtype=np.float64)[held], cd])
            ci = np.concatenate([np.asarray(mi[i], dtype=np.int64)[held], ci])
        order = np.lexsort((ci, cd))[:k]
        out_d[i, :order.size] = cd[order]
        out_i[i, :order.size] = ci[order]
        count[i] = order.size
    return out_d, out_i, count
