"""`pyatac motifs`: the sites of transcription-factor motifs in a genome or in the windows of a BED file, and the window-by-motif match
matrix.  This command is this package's own, like `peaks` and `cellcounts`: the reference has no motif scanner.  `pyatac signal --bed`,
`pyatac nucleotide --bed` and `cellqc --tss` aggregate around sites; this command makes such sites from a motif file and the FASTA alone,
and its matrix (rows the windows, columns the motifs) is the partner of the `cellcounts` matrix for motif enrichment per cluster.

The rule (include/natac.h states the device's part).

Host, once per run.  --motifs is MEME minimal text (`MOTIF id [alt]`, `letter-probability matrix: alength= 4 w= W nsites= N`, W rows of
A C G T probabilities; nsites is 20 when absent; counts = prob * nsites) or JASPAR (`>id [alt]`, four rows `A [ c c ... ]`, C, G, T of
counts); the format is told from the first non-empty line that is not a `#` comment.  A malformed file stops the command with
`<path>: line <N>: <reason>`.  1 <= W <= 64, ids match [A-Za-z0-9._:-]{1,64} and are unique, at most 4096 motifs; --only keeps the listed
ids in file order.  Background: --bg uniform (0.25 each), --bg a c g t (four positive numbers that sum to 1 within 1e-6) or --bg regions
(the A/C/G/T of the scan intervals counted by natac_base_counts, made strand-symmetric: A = T = (nA + nT) / 2N, C = G = (nC + nG) / 2N).
Integer scores: p[j][b] = (c[j][b] + pc bg[b]) / (sum_b c[j][b] + pc) with pc = --pseudocount, S[j][b] = rint(100 log2(p[j][b] / bg[b]))
as int32: 0.01 bit is the resolution of everything after this step.  Threshold: the exact distribution of the integer score of one window
under the i.i.d. background, by convolving the columns in fp64 over an array indexed by score - sum_j min_b S[j][b]; tail probabilities
are summed from the top score downwards; T is the smallest integer t with P(score >= t) <= --pvalue.  If not even the maximum score
satisfies that (short motifs), T = max + 1: the motif has no hit and the summary says NA.

Device, one natac_motif_scan call per chromosome with windows (csrc/natac_motifs.hpp), integers only.  The BED windows that overlap or
abut are merged into scan intervals (without --bed the one window is the chromosome).  A motif of width W is scored at x when [x, x + W)
lies inside one scan interval and all W bases are ACGT: fwd = sum_j S[j][code(seq[x + j])], rev = sum_j S[W - 1 - j][3 - code(seq[x + j])];
a `+` hit is fwd >= T, a `-` hit rev >= T.  The hits come back sorted by (motif, start, strand), each site once however many windows
cover it; the matrix entry (window i, motif m) is the number of hits with start_i <= x and x + W_m <= end_i, counted per window.

BASE.motifs.sites.bed.gz   chrom start end id score strand, score = the integer score / 100 written %.2f; ordered by motif (file order),
                           chromosome (FASTA order), start, `+` before `-`; BGZF without an index.  `pyatac signal --bed ... --strand 6`
                           and `pyatac nucleotide --bed ... --strand 6` take it unchanged; --only ID makes it one factor's site list.
BASE.motifs.mtx.gz + .names.tsv (id TAB alt) + .regions.bed (--format mtx), or BASE.motifs.npz (CSR: indptr, indices, data, shape, motifs,
                           region_chrom, region_start, region_end): the layout of the `cellcounts` files.
BASE.motifs.txt            the background, the p-value and the pseudocount; per motif id alt width max_score threshold tail_p hits_plus
                           hits_minus windows_hit (tail_p = the probability reached at T; threshold and tail_p NA when unreachable);
                           then bases_scanned, scan_intervals, windows and hits.
Everything is computed before the first file is written, so an error leaves nothing behind; no hit at all is not an error.

Measured on the MI355X box (tools/bench_motifs.py, one box, one process, three runs after a warm-up call: 4 chromosomes of 50 Mbp,
100,000 non-overlapping 500-base windows, 500 random count matrices of 8 to 20 columns, p = 1e-4; 3.42e11 column look-ups, 4.80 M hits,
4.57 M matrix entries): the four device calls 0.164 s in the first run and 0.107 / 0.091 s in the next two (table building, upload,
download included; 49.9 ms between their first and last kernels, 41 ms of it the scan kernel by a kernel trace of a separate run):
6.9e12 look-ups a second, about two fifths of the LDS's ds_read_b32 rate (32 lanes x 256 CUs x 2.4 GHz).  The NumPy restatement of
tests/motifs_ref.py on 100 of the 100,000 windows (0.1 %) on that box: 2.6 s, and equal.
"""
import gzip
import os
import re
import time
import warnings

import numpy as np

SCALE = 100                # NATAC_MOTIF_SCALE
ID_RE = re.compile(r"^[A-Za-z0-9._:-]{1,64}$")
BASES = "ACGT"


class MotifsError(ValueError):
    """`pyatac motifs` cannot answer: a malformed motif file, arguments that break a rule, a missing file, a window past its chromosome"""


# ---- the motif file -------------------------------------------------------------------------------------------------------------
def _numbers(tokens):
    try:
        v = [float(t) for t in tokens]
    except ValueError:
        return None
    return v if all(np.isfinite(x) and x >= 0 for x in v) else None


def _parse_meme(path, lines):
    motifs = []
    i, n = 0, len(lines)
    while i < n:
        f = lines[i].split()
        if not f or f[0] != "MOTIF":
            i += 1
            continue
        head = i + 1
        if len(f) < 2:
            raise MotifsError("%s: line %d: MOTIF without an id" % (path, head))
        mid, alt = f[1], " ".join(f[2:])
        i += 1
        while i < n and not lines[i].strip():
            i += 1
        if i >= n or not lines[i].strip().startswith("letter-probability matrix"):
            raise MotifsError("%s: line %d: motif %s has no letter-probability matrix" % (path, min(i, n - 1) + 1, mid))
        keys = dict(re.findall(r"(\w+)=\s*(\S+)", lines[i]))
        try:
            alength = int(keys.get("alength", 4))
            w = int(keys["w"]) if "w" in keys else None
            nsites = float(keys.get("nsites", 20))
        except ValueError:
            raise MotifsError("%s: line %d: motif %s: unreadable matrix header" % (path, i + 1, mid))
        if alength != 4:
            raise MotifsError("%s: line %d: motif %s: alength is %d, not 4" % (path, i + 1, mid, alength))
        if not nsites > 0 or not np.isfinite(nsites):
            raise MotifsError("%s: line %d: motif %s: nsites must be positive" % (path, i + 1, mid))
        i += 1
        rows = []
        while i < n and (w is None or len(rows) < w):
            v = _numbers(lines[i].split())
            if v is None or len(v) != 4:
                if w is None:
                    break
                raise MotifsError("%s: line %d: motif %s: expected row %d of %d with four probabilities" % (path, i + 1, mid, len(rows) + 1, w))
            if abs(sum(v) - 1.0) > 0.01:
                raise MotifsError("%s: line %d: motif %s: the probabilities sum to %.4g, not 1" % (path, i + 1, mid, sum(v)))
            rows.append(v)
            i += 1
        if w is not None and len(rows) < w:
            raise MotifsError("%s: line %d: motif %s: the file ends after %d of %d rows" % (path, n, mid, len(rows), w))
        motifs.append((mid, alt, np.array(rows, np.float64).reshape(-1, 4) * nsites, head))
    return motifs


def _parse_jaspar(path, lines):
    motifs = []
    i, n = 0, len(lines)
    while i < n:
        s = lines[i].strip()
        if not s or s.startswith("#"):
            i += 1
            continue
        if not s.startswith(">"):
            raise MotifsError("%s: line %d: expected a `>id` header" % (path, i + 1))
        f = s[1:].split()
        head = i + 1
        if not f:
            raise MotifsError("%s: line %d: header without an id" % (path, head))
        mid, alt = f[0], " ".join(f[1:])
        rows = []
        i += 1
        for b in BASES:
            while i < n and not lines[i].strip():
                i += 1
            if i >= n:
                raise MotifsError("%s: line %d: motif %s: the file ends before row %s" % (path, n, mid, b))
            tok = lines[i].replace("[", " ").replace("]", " ").split()
            if tok and tok[0].upper() in BASES and len(tok[0]) == 1:
                if tok[0].upper() != b:
                    raise MotifsError("%s: line %d: motif %s: expected row %s, found row %s" % (path, i + 1, mid, b, tok[0]))
                tok = tok[1:]
            v = _numbers(tok)
            if v is None:
                raise MotifsError("%s: line %d: motif %s: row %s is not a row of counts" % (path, i + 1, mid, b))
            if rows and len(v) != len(rows[0]):
                raise MotifsError("%s: line %d: motif %s: row %s has %d columns, row A has %d" % (path, i + 1, mid, b, len(v), len(rows[0])))
            rows.append(v)
            i += 1
        motifs.append((mid, alt, np.array(rows, np.float64).reshape(4, -1).T.copy(), head))
    return motifs


def parse_motifs(path):
    """[(id, alt, counts float64[W, 4])] of a MEME or JASPAR file, in file order -> MotifsError `<path>: line <N>: <reason>`"""
    from .._lib import MOTIF_MAX_MOTIFS, MOTIF_MAX_WIDTH
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as fh:
        lines = fh.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()                                   # the file ends with a newline: no line behind it
    first = next((k for k, s in enumerate(lines) if s.strip() and not s.lstrip().startswith("#")), None)
    if first is None:
        raise MotifsError("%s: line %d: no motif in the file" % (path, max(len(lines), 1)))
    s = lines[first].lstrip()
    if s.startswith(">"):
        motifs = _parse_jaspar(path, lines)
    elif s.startswith("MEME") or s.startswith("MOTIF"):
        motifs = _parse_meme(path, lines)
    else:
        raise MotifsError("%s: line %d: neither a MEME (`MEME version`, `MOTIF`) nor a JASPAR (`>id`) file" % (path, first + 1))
    if not motifs:
        raise MotifsError("%s: line %d: no motif in the file" % (path, first + 1))
    seen = {}
    for k, (mid, _alt, counts, head) in enumerate(motifs):
        if not ID_RE.match(mid):
            raise MotifsError("%s: line %d: motif id %r does not match [A-Za-z0-9._:-]{1,64}" % (path, head, mid))
        if mid in seen:
            raise MotifsError("%s: line %d: motif id %s is already used at line %d" % (path, head, mid, seen[mid]))
        seen[mid] = head
        if not 1 <= counts.shape[0] <= MOTIF_MAX_WIDTH:
            raise MotifsError("%s: line %d: motif %s: width %d is outside 1 .. %d" % (path, head, mid, counts.shape[0], MOTIF_MAX_WIDTH))
        if k >= MOTIF_MAX_MOTIFS:
            raise MotifsError("%s: line %d: motif %s: more than %d motifs" % (path, head, mid, MOTIF_MAX_MOTIFS))
    return [(mid, alt, counts) for mid, alt, counts, _ in motifs]


# ---- scores and thresholds ------------------------------------------------------------------------------------------------------
def scores(counts, bg, pseudocount):
    """int32[W, 4]: S[j][b] = rint(100 log2(p / bg[b])), p = (c[j][b] + pc bg[b]) / (sum_b c[j][b] + pc)"""
    c = np.asarray(counts, np.float64)
    bg = np.asarray(bg, np.float64)
    p = (c + pseudocount * bg) / (c.sum(axis=1, keepdims=True) + pseudocount)
    return np.rint(SCALE * np.log2(p / bg)).astype(np.int32)


def score_distribution(S, bg):
    """(dist float64[max - min + 1], min): dist[k] = P(score = min + k) of one window under the i.i.d. background"""
    S = np.asarray(S, np.int64)
    lo = S.min(axis=1)
    dist = np.ones(1, np.float64)
    for j in range(S.shape[0]):
        new = np.zeros(len(dist) + int(S[j].max() - lo[j]), np.float64)
        for b in range(4):
            d = int(S[j, b] - lo[j])
            new[d:d + len(dist)] += bg[b] * dist
        dist = new
    return dist, int(lo.sum())


def threshold(S, bg, pvalue):
    """(T, tail_p, max_score): T the smallest integer t with P(score >= t) <= pvalue, tail_p the probability reached there; T = max + 1
    and tail_p None when not even the maximum score satisfies it"""
    dist, lo = score_distribution(S, bg)
    tail = np.cumsum(dist[::-1])[::-1]                   # summed from the top score downwards
    top = lo + len(dist) - 1
    k = int(np.argmax(tail <= pvalue)) if tail[-1] <= pvalue else None
    if k is None:
        return top + 1, None, top
    return lo + k, float(tail[k]), top


def parse_bg(tokens):
    """--bg -> "uniform", "regions" or float64[4]"""
    tokens = list(tokens) if tokens else ["uniform"]
    if len(tokens) == 1 and tokens[0] in ("uniform", "regions"):
        return tokens[0]
    try:
        v = np.array([float(t) for t in tokens], np.float64)
    except ValueError:
        v = None
    if v is None or v.shape != (4,) or not np.all(np.isfinite(v)) or not np.all(v > 0) or abs(v.sum() - 1.0) > 1e-6:
        raise MotifsError("--bg takes `uniform`, `regions` or four positive numbers a c g t that sum to 1 (got %s)" % " ".join(tokens))
    return v


def merge_intervals(start, end):
    """the scan intervals of the windows: (start, end) int64, ascending, windows that overlap or abut merged, empty ones dropped"""
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    keep = end > start
    start, end = start[keep], end[keep]
    if not len(start):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    order = np.argsort(start, kind="stable")
    s, e = start[order], np.maximum.accumulate(end[order])
    head = np.ones(len(s), bool)
    head[1:] = s[1:] > e[:-1]
    first = np.flatnonzero(head)
    return s[first], e[np.append(first[1:] - 1, len(s) - 1)]


# ---- the command ----------------------------------------------------------------------------------------------------------------
def check_args(args):
    if not 0 < args.pvalue < 1:
        raise MotifsError("--pvalue (%s) must lie strictly between 0 and 1" % args.pvalue)
    if not args.pseudocount > 0 or not np.isfinite(args.pseudocount):
        raise MotifsError("--pseudocount (%s) must be positive" % args.pseudocount)
    if args.format not in ("mtx", "npz"):
        raise MotifsError("--format must be mtx or npz (got %s)" % args.format)
    return parse_bg(args.bg)


def read_windows(bed, fasta):
    """(chrom int32 = index into fasta.references, start, end) of the BED rows in file order, zero-length rows dropped, rows on
    chromosomes the FASTA lacks dropped with one warning; without a BED every chromosome whole"""
    if bed is None:
        return (np.arange(len(fasta.references), dtype=np.int32), np.zeros(len(fasta.references), np.int64),
                np.array(fasta.lengths, np.int64))
    from .chunk import read_bed_columns
    names, chrom, start, end, _ = read_bed_columns(bed)
    index = {c: k for k, c in enumerate(fasta.references)}
    to_fasta = np.array([index.get(c, -1) for c in names], np.int32) if names else np.zeros(0, np.int32)
    fc = to_fasta[chrom] if len(chrom) else np.zeros(0, np.int32)
    bad = sorted(set(np.array(names, dtype=object)[chrom[fc < 0]].tolist())) if len(chrom) else []
    if bad:
        warnings.warn("%d chromosome names in %s not included in the fasta file:\n%s\n Regions on these chromosomes will be ignored"
                      % (len(bad), bed, "\n".join(bad)))
    keep = fc >= 0
    fc, start, end = fc[keep], start[keep], end[keep]
    lengths = np.array(fasta.lengths, np.int64)
    past = np.flatnonzero((start < 0) | (end > lengths[fc])) if len(fc) else []
    if len(past):
        i = int(past[0])
        raise MotifsError("%s: the window %s:%d-%d reaches past the chromosome (%d bases)"
                          % (bed, fasta.references[int(fc[i])], start[i], end[i], lengths[fc[i]]))
    return fc, start, end


def scan(fasta, fc, start, end, widths, S_flat, T, timing=None):
    """one natac_motif_scan call per chromosome with windows, FASTA order -> (hits = (chrom, motif, start, strand, score) ordered by motif,
    chromosome, start, strand; CSR (indptr, indices, data) of the window-by-motif counts, rows in the windows' order)"""
    from .. import get_context
    t = timing if timing is not None else {}
    t.setdefault("device_s", 0.0)
    t.setdefault("kernel_ms", 0.0)
    M, n_rows = len(widths), len(start)
    per_chrom, parts = [], []
    row_nnz = np.zeros(n_rows, np.int64)
    for k, c in enumerate(fasta.references):
        idx = np.flatnonzero(fc == k)
        if not len(idx) or not M:
            continue
        t0 = time.perf_counter()
        hm, hs, hst, hsc, cnt, ms = get_context().motif_scan(fasta.seqs[c], start[idx], end[idx], widths, S_flat, T, with_kernel_ms=True)
        t["device_s"] += time.perf_counter() - t0
        t["kernel_ms"] += ms
        per_chrom.append((k, hm, hs, hst, hsc))
        r, m = np.nonzero(cnt)                               # row-major: by row, then by motif
        ptr = np.zeros(len(idx) + 1, np.int64)
        np.cumsum(np.bincount(r, minlength=len(idx)), out=ptr[1:])
        row_nnz[idx] = np.diff(ptr)
        parts.append((idx, ptr, m.astype(np.int32), cnt[r, m].astype(np.int32)))
    indptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(row_nnz, out=indptr[1:])
    indices = np.empty(int(indptr[-1]), np.int32)
    data = np.empty(int(indptr[-1]), np.int32)
    for idx, ptr, col, val in parts:             # entry q of the chromosome's row j goes to indptr[idx[j]] + (q - ptr[j])
        dest = np.repeat(indptr[idx] - ptr[:-1], np.diff(ptr)) + np.arange(len(col), dtype=np.int64)
        indices[dest] = col
        data[dest] = val
    # the hits of every chromosome are sorted by motif: their stretches are put side by side per motif, nothing is sorted
    bounds = [np.searchsorted(hm, np.arange(M + 1)) for _, hm, _, _, _ in per_chrom]
    per = np.array([np.diff(b) for b in bounds], np.int64).reshape(len(per_chrom), M)       # [chromosome, motif]
    first = np.zeros(per.size + 1, np.int64)
    np.cumsum(per.T.ravel(), out=first[1:])                  # (motif, chromosome) order
    first = first[:-1].reshape(M, len(per_chrom)).T
    total = int(per.sum())
    out = (np.empty(total, np.int32), np.empty(total, np.int32), np.empty(total, np.int64), np.empty(total, np.uint8), np.empty(total, np.int32))
    for q, (k, hm, hs, hst, hsc) in enumerate(per_chrom):
        dest = np.repeat(first[q] - bounds[q][:-1], per[q]) + np.arange(len(hm), dtype=np.int64)
        out[0][dest] = k
        for o, a in zip(out[1:], (hm, hs, hst, hsc)):
            o[dest] = a
    return out, (indptr, indices, data)


def get_motifs(args, timing=None):
    """`pyatac motifs`: writes BASE.motifs.sites.bed.gz (unless --no_sites), the matrix files and BASE.motifs.txt; returns
    dict(hits, matrix, motifs, table, bg)"""
    from .get_cellcounts import mtx_text
    from .seq import FastaStore
    bg = check_args(args)
    for path in (args.fasta, args.motifs, args.bed):
        if path is not None and not os.path.exists(path):
            raise MotifsError("%s: no such file" % path)
    base = (args.out if args.out is not None else ".".join(os.path.basename(args.motifs).split(".")[0:-1])) + ".motifs"
    t = timing if timing is not None else {}
    motifs = parse_motifs(args.motifs)
    if args.only:
        have = {m[0] for m in motifs}
        unknown = [i for i in args.only if i not in have]
        if unknown:
            raise MotifsError("--only: no motif %s in %s" % (", ".join(unknown), args.motifs))
        motifs = [m for m in motifs if m[0] in set(args.only)]
    fasta = FastaStore.open(args.fasta)
    fc, start, end = read_windows(args.bed, fasta)
    # the scan intervals, and the background
    n_iv = bases = 0
    acgt = np.zeros(4, np.int64)
    for k, c in enumerate(fasta.references):
        idx = np.flatnonzero(fc == k)
        s, e = merge_intervals(start[idx], end[idx])
        n_iv += len(s)
        bases += int((e - s).sum())
        if isinstance(bg, str) and bg == "regions" and len(s):
            from .. import get_context
            acgt += get_context().base_counts(fasta.seqs[c], s, e)
    if isinstance(bg, str):
        if bg == "regions":
            if acgt.sum() == 0:
                raise MotifsError("--bg regions: the scan intervals hold no A, C, G or T")
            at, cg = (acgt[0] + acgt[3]) / (2.0 * acgt.sum()), (acgt[1] + acgt[2]) / (2.0 * acgt.sum())
            bg_used = np.array([at, cg, cg, at], np.float64)
            if not np.all(bg_used > 0):
                raise MotifsError("--bg regions: a base does not occur in the scan intervals")
        else:
            bg_used = np.full(4, 0.25)
    else:
        bg_used = bg
    S_list = [scores(m[2], bg_used, args.pseudocount) for m in motifs]
    thr = [threshold(S, bg_used, args.pvalue) for S in S_list]
    widths = np.array([len(S) for S in S_list], np.int32)
    S_flat = np.concatenate(S_list).astype(np.int32) if S_list else np.zeros((0, 4), np.int32)
    T = np.array([x[0] for x in thr], np.int32)
    hits, (indptr, indices, data) = scan(fasta, fc, start, end, widths, S_flat, T, timing=t)
    h_chrom, h_motif, h_start, h_strand, h_score = hits
    M = len(motifs)
    plus = np.bincount(h_motif[h_strand == 0], minlength=M)
    minus = np.bincount(h_motif[h_strand == 1], minlength=M)
    win_hit = np.bincount(indices, minlength=M)
    # ---- texts, then files
    lines = ["background\t%s\t%s\n" % (bg if isinstance(bg, str) else "given", "\t".join("%.6f" % x for x in bg_used)),
             "pvalue\t%g\npseudocount\t%g\n" % (args.pvalue, args.pseudocount),
             "id\talt\twidth\tmax_score\tthreshold\ttail_p\thits_plus\thits_minus\twindows_hit\n"]
    for k, (mid, alt, _counts) in enumerate(motifs):
        Tk, tail, top = thr[k]
        lines.append("%s\t%s\t%d\t%.2f\t%s\t%s\t%d\t%d\t%d\n" % (mid, alt, widths[k], top / float(SCALE), "NA" if tail is None else "%.2f" % (Tk / float(SCALE)),
                                                              "NA" if tail is None else "%.6g" % tail, plus[k], minus[k], win_hit[k]))
    lines.append("bases_scanned\t%d\nscan_intervals\t%d\nwindows\t%d\nhits\t%d\n" % (bases, n_iv, len(start), len(h_motif)))
    summary = "".join(lines)
    ids = [m[0] for m in motifs]
    region_chrom = np.array(fasta.references, dtype=object)[fc] if len(fc) else np.zeros(0, dtype=object)
    t0 = time.perf_counter()
    if not args.no_sites:
        from ..writer import bgzip_file, write_bed_rows
        w_of = widths.astype(np.int64)[h_motif] if len(h_motif) else np.zeros(0, np.int64)
        lo = int(h_score.min()) if len(h_score) else 0
        span = (int(h_score.max()) - lo + 1) if len(h_score) else 1
        key = (h_motif.astype(np.int64) * span + (h_score.astype(np.int64) - lo)) * 2 + h_strand
        uniq, label_id = np.unique(key, return_inverse=True)
        labels = ["%s\t%.2f\t%s" % (ids[int(u // 2 // span)], ((u // 2) % span + lo) / float(SCALE), "+-"[int(u % 2)]) for u in uniq.tolist()]
        txt = base + ".sites.bed"
        if len(h_motif):
            write_bed_rows(txt, fasta.references, h_chrom, h_start, h_start + w_of, np.zeros((len(h_motif), 0)), append=False,
                           labels=labels, label_id=label_id)
        else:
            open(txt, "w").close()
        bgzip_file(txt)
    if args.format == "npz":
        np.savez_compressed(base + ".npz", indptr=indptr, indices=indices, data=data, shape=np.array([len(start), M], np.int64),
                            motifs=np.array(ids, dtype="S"), alts=np.array([m[1] for m in motifs], dtype="U"),
                            region_chrom=region_chrom.astype("U"), region_start=start, region_end=end)
    else:
        text = mtx_text(indptr, indices, data, M)
        bed = "".join(["%s\t%d\t%d\n" % r for r in zip(region_chrom.tolist(), start.tolist(), end.tolist())])
        with gzip.open(base + ".mtx.gz", "wb") as f:
            f.write(text)
        with open(base + ".names.tsv", "w") as f:
            f.write("".join("%s\t%s\n" % (m[0], m[1]) for m in motifs))
        with open(base + ".regions.bed", "w") as f:
            f.write(bed)
    with open(base + ".txt", "w") as f:
        f.write(summary)
    t["write_s"] = time.perf_counter() - t0
    return dict(hits=hits, matrix=(indptr, indices, data), motifs=motifs, table=thr, bg=bg_used, widths=widths, scores=S_flat, thresholds=T)
