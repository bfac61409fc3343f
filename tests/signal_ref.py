"""NumPy restatement of `pyatac signal` (the reference's pyatac/signal_around_sites.py:24-118 with bedgraph.py:6-14 and
chunk.py:26-54), written from the rule and not from the kernels: what the tests compare natac_site_signal and get_signal with, and
what tools/bench_sites.py signal times."""
import numpy as np

EXP, POSITIVE, SCALE = 1, 2, 4


def site_window(start, end, minus, up, down, size):
    """one site: (centre, clipped window start, clipped window end, zero columns before it in genomic orientation); Python-2
    integer division for the centre; the centre is extended only when up and down are both non-zero"""
    half = (end - start) // 2
    c = end - half - 1 if minus else start + half
    if up == 0 or down == 0:
        return c, c, c + 1, 0
    ws = max(0, c - (down if minus else up))
    we = min(size, c + 1 + (up if minus else down))
    K = up + down + 1
    return c, ws, we, (K - (we - ws) if ws == 0 else 0)


def read_track(records, chrom, s, e):
    """BedGraphFile.read: e - s values, NaN where no record of `records` [(chrom, begin, end, value), ...] covers a base, else the
    value of the last covering record in list order"""
    out = np.full(max(e - s, 0), np.nan)
    for c, b, z, v in records:
        if c == chrom and z > s and b < e:
            out[max(b - s, 0):min(z - s, e - s)] = v
    return out


def transform(row, flags):
    """one row already padded and in strand orientation (a copy is returned)"""
    sig = np.array(row, dtype=np.float64)
    if flags & EXP:
        sig = np.exp(sig)
    if flags & POSITIVE:
        sig[sig < 0] = 0
    if flags & SCALE:
        sig[np.isnan(sig)] = 0
        s = np.sum(np.abs(sig))
        sig = sig / (s + (s == 0))
    return sig


def rows_ref(vals, src, length, lead, minus, K, flags):
    """the matrix natac_site_signal is asked for: row i = lead[i] zeros, vals[src[i] : src[i] + length[i]], zeros up to K; reversed
    where minus[i]; transformed"""
    n = len(src)
    mat = np.zeros((n, K))
    for i in range(n):
        g = np.zeros(K)
        g[lead[i]:lead[i] + length[i]] = vals[src[i]:src[i] + length[i]]
        if minus is not None and minus[i]:
            g = g[::-1]
        mat[i] = transform(g, flags)
    return mat


def rows_ref_fast(vals, src, length, lead, minus, K, flags):
    """rows_ref with whole-matrix NumPy operations (for large inputs): the same values, except that --scale's row sums are
    np.sum along the rows"""
    n = len(src)
    j = np.arange(K)[None, :]
    rev = np.zeros(n, bool) if minus is None else np.asarray(minus, bool)
    rel = np.where(rev[:, None], K - 1 - j, j) - np.asarray(lead)[:, None]
    inside = (rel >= 0) & (rel < np.asarray(length)[:, None])
    idx = np.where(inside, np.asarray(src)[:, None] + rel, 0)
    mat = np.where(inside, np.asarray(vals)[idx] if len(vals) else 0.0, 0.0)
    if flags & EXP:
        mat = np.exp(mat)
    if flags & POSITIVE:
        mat[mat < 0] = 0
    if flags & SCALE:
        mat[np.isnan(mat)] = 0
        s = np.sum(np.abs(mat), axis=1)
        mat = mat / (s + (s == 0))[:, None]
    return mat


def aggregate(mat):
    """the reference's aggregate: the column sum with NaN as 0"""
    m = np.array(mat)
    m[np.isnan(m)] = 0
    return np.sum(m, axis=0)


def aggregate_in_segments(mat, seg):
    """the documented order of natac_site_signal: NaN as 0; a column is added site by site from 0 inside every segment of `seg`
    consecutive sites, then the segment sums are added in order from 0"""
    m = np.array(mat)
    m[np.isnan(m)] = 0
    total = np.zeros(m.shape[1])
    for a in range(0, len(m), seg):
        part = np.zeros(m.shape[1])
        for row in m[a:a + seg]:
            part = part + row
        total = total + part
    return total


def signal_ref(records, sizes, sites, up, down, flags):
    """the matrix of `pyatac signal --all` for sites [(chrom, start, end, minus), ...] (rows of length < 1 already dropped)"""
    K = up + down + 1
    mat = np.zeros((len(sites), K))
    for i, (chrom, start, end, minus) in enumerate(sites):
        _, ws, we, lead = site_window(start, end, minus, up, down, sizes.get(chrom, 0))
        g = np.zeros(K)
        g[lead:lead + we - ws] = read_track(records, chrom, ws, we)
        mat[i] = transform(g[::-1] if minus else g, flags)
    return mat
