"""NumPy restatements of the two counting rules behind `pyatac counts` and `pyatac nucleotide` (pyatac/get_counts.py:30-45;
get_nucleotide.py:19-38 with chunk.center / slop and seq.get_sequence / seq_to_mat), written from the reference's rules, not from
the kernels: what the GPU tests compare natac_region_counts and natac_site_seq_counts with, and what tools/bench_sites.py times."""
import itertools

import numpy as np

ACGT = ["A", "C", "G", "T"]
DINUCLEOTIDES = ["".join(p) for p in itertools.product("CGAT", repeat=2)]


def fragment_ends(pos, tlen, atac):
    pos, tlen = np.asarray(pos, np.int64), np.asarray(tlen, np.int64)
    l, ilen = (pos + 4, tlen - 8) if atac else (pos, tlen)
    return l, ilen, l + ilen - 1


def region_counts_brute(pos, tlen, starts, ends, lower, upper, atac):
    """every record tested against every region"""
    l, ilen, r = fragment_ends(pos, tlen, atac)
    ok = (ilen >= lower) & (ilen < upper)
    l, r = l[ok], r[ok]
    return np.array([int(np.count_nonzero(((l >= s) & (l < e)) | ((r >= s) & (r < e)))) for s, e in zip(starts, ends)], np.int64)


def region_counts_ref(pos, tlen, starts, ends, lower, upper, atac):
    """the same, testing per region only the records whose left end lies within upper + |lower| + 16 of it (pos is sorted)"""
    l, ilen, r = fragment_ends(pos, tlen, atac)
    ok = (ilen >= lower) & (ilen < upper)
    margin = abs(int(upper)) + abs(int(lower)) + 16
    a = np.searchsorted(l, np.asarray(starts, np.int64) - margin, "left")
    b = np.searchsorted(l, np.asarray(ends, np.int64) + margin, "right")
    out = np.zeros(len(starts), np.int64)
    for i, (s, e) in enumerate(zip(starts, ends)):
        ll, rr = l[a[i]:b[i]], r[a[i]:b[i]]
        out[i] = np.count_nonzero(ok[a[i]:b[i]] & (((ll >= s) & (ll < e)) | ((rr >= s) & (rr < e))))
    return out


def site_window(center, minus, up, down, word, n):
    """(start, end, used): the clipped window of chunk.slop(up, down + word - 1) around [center, center + 1)"""
    lo, hi = (down + word - 1, up) if minus else (up, down + word - 1)
    s, e = max(0, center - lo), min(n, center + 1 + hi)
    return s, e, e - s == up + down + word


_PLUS = np.full(256, 4, np.uint8)
_MINUS = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _PLUS[ord(_c)] = _PLUS[ord(_c.lower())] = _i
    _MINUS[ord(_c)] = 3 - _i               # translate('ACGT' -> 'TGCA') runs before upper(): upper case is complemented,
    _MINUS[ord(_c.lower())] = _i           # lower case is not
_CGAT = np.array([2, 0, 1, 3, 4])          # A C G T -> place in "CGAT"


def site_counts_ref(seq, centers, minus, up, down, word, step=1024):
    """(M int64[4 or 16, up + down + 1], n used) over the sites of one chromosome"""
    seq = np.asarray(seq, np.uint8)
    n, K, d = len(seq), up + down + 1, word - 1
    centers = np.asarray(centers, np.int64)
    minus = np.zeros(len(centers), bool) if minus is None else np.asarray(minus, bool)
    w0 = np.where(minus, centers - down - d, centers - up)
    w1 = np.where(minus, centers + up + 1, centers + down + 1 + d)
    used = (w0 >= 0) & (w1 <= n)
    R = 16 if word == 2 else 4
    M = np.zeros(R * K, np.int64)
    j = np.arange(K + d)
    for rev, table in ((False, _PLUS), (True, _MINUS)):
        c = centers[used & (minus == rev)]
        for o in range(0, len(c), step):
            cc = c[o:o + step, None]
            code = table[seq[(cc + up - j) if rev else (cc - up + j)]].astype(np.int64)      # [sites, K + d]: the strand's string
            if word == 2:
                a, b = _CGAT[code[:, :-1]], _CGAT[code[:, 1:]]
                row = np.where((a < 4) & (b < 4), 4 * a + b, R)
            else:
                row = np.where(code < 4, code, R)
            flat = (row * K + np.arange(K))[row < R]
            M += np.bincount(flat, minlength=R * K)
    return M.reshape(R, K), int(used.sum())


def fasta_text(names, seqs, width):
    out = []
    for c in names:
        raw = bytes(np.asarray(seqs[c], np.uint8))
        out.append(b">" + c.encode() + b"\n" + b"".join(raw[i:i + width] + b"\n" for i in range(0, len(raw), width)))
    return b"".join(out)
