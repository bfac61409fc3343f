"""NumPy restatement of the whole rule of `pyatac deviations` (nucleoatac_amd/pyatac/get_deviations.py, include/natac.h), the background
table included, on dense matrices: slow, plain and independent of the package's own host code.  It loops over b and is vectorised over
the cells.  The tests compare the device entry, the command's host code and the files it writes against this module; test_deviations_host.py
compares this module itself with exact rationals."""
import gzip
import io
import zipfile

import numpy as np


def grid_shape(P, gc_bins, acc_bins, min_bin):
    n_g, n_a = gc_bins, acc_bins
    while P // (n_g * n_a) < min_bin and n_g * n_a > 1:
        if n_g > n_a:
            n_g -= 1
        else:
            n_a -= 1
    return n_g, n_a


def candidates(gc, rs, n_g, n_a):
    """cand[p] = the ascending window indices of the grid cell of window p (a list shared by the cell's windows)"""
    P = len(gc)
    by_gc = sorted(range(P), key=lambda p: (gc[p], p))
    cand = [None] * P
    for k in range(n_g):
        members = by_gc[(k * P) // n_g:((k + 1) * P) // n_g]
        by_rs = sorted(members, key=lambda p: (rs[p], p))
        L = len(by_rs)
        for j in range(n_a):
            part = sorted(by_rs[(j * L) // n_a:((j + 1) * L) // n_a])
            for p in part:
                cand[p] = part
    return cand


def background(gc, rs, B, gc_bins=25, acc_bins=25, min_bin=10, seed=1):
    """(bg int64[B + 1, P] with bg[0] the identity, (n_g, n_a), (smallest, largest cell))"""
    P = len(gc)
    n_g, n_a = grid_shape(P, gc_bins, acc_bins, min_bin)
    cand = candidates([float(g) for g in gc], [int(v) for v in rs], n_g, n_a)
    r = np.random.default_rng(seed).random((B, P))
    bg = np.empty((B + 1, P), np.int64)
    bg[0] = np.arange(P)
    for b in range(1, B + 1):
        for p in range(P):
            bg[b, p] = cand[p][int(r[b - 1, p] * len(cand[p]))]
    sizes = [len(c) for c in cand]
    return bg, (n_g, n_a), (min(sizes), max(sizes))


def sums(X, sets, bg):
    """O int64[B + 1, M, N] and E int64[B + 1, M] of the dense live matrix X [P, N], the motifs' window sets and bg [B + 1, P]"""
    X = np.asarray(X, np.int64)
    rs = X.sum(axis=1)
    O = np.zeros((bg.shape[0], len(sets), X.shape[1]), np.int64)
    E = np.zeros((bg.shape[0], len(sets)), np.int64)
    for b in range(bg.shape[0]):
        for m, s in enumerate(sets):
            rows = bg[b][np.asarray(s, np.int64)]
            O[b, m] = X[rows].sum(axis=0)
            E[b, m] = rs[rows].sum()
    return O, E


def statistics(O, E, d, T):
    """(raw, bg_mean, bg_m2, s): fp64, one rounded operation at a time; s = 1 + max over b of |Y_b| per element"""
    B = O.shape[0] - 1
    d = np.asarray(d, np.int64).astype(np.float64)
    Tf = np.float64(T)
    raw = None
    mean = np.zeros(O.shape[1:], np.float64)
    m2 = np.zeros(O.shape[1:], np.float64)
    big = np.zeros(O.shape[1:], np.float64)
    for b in range(B + 1):
        x = E[b].astype(np.float64)[:, None] * d[None, :]
        x = x / Tf
        Y = (O[b].astype(np.float64) - x) / x
        big = np.maximum(big, np.abs(Y))
        if b == 0:
            raw = Y
            continue
        delta = Y - mean
        mean = mean + delta / np.float64(b)
        m2 = m2 + delta * (Y - mean)
    return raw, mean, m2, 1.0 + big


def deviations(X, H, gc, B=50, gc_bins=25, acc_bins=25, min_bin=10, seed=1):
    """the whole rule on the dense count matrix X [windows, cells], the dense hit matrix H [windows, motifs] and gc per window"""
    X, H = np.asarray(X, np.int64), np.asarray(H, np.int64)
    win_keep, cell_keep = X.sum(axis=1) > 0, X.sum(axis=0) > 0
    Xl = X[win_keep][:, cell_keep]
    Hl = H[win_keep] > 0
    motif_keep = Hl.sum(axis=0) > 0
    sets = [np.flatnonzero(Hl[:, m]) for m in np.flatnonzero(motif_keep)]
    rs, d, T = Xl.sum(axis=1), Xl.sum(axis=0), int(Xl.sum())
    bg, grid, extremes = background(np.asarray(gc, np.float64)[win_keep], rs, B, gc_bins, acc_bins, min_bin, seed)
    O, E = sums(Xl, sets, bg)
    raw, mean, m2, s = statistics(O, E, d, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(m2 / np.float64(B - 1))
        dev = raw - mean
        z = dev / sd
    z[sd == 0] = np.nan
    var = np.full(len(sets), np.nan)
    for m in range(len(sets)):
        ok = z[m][np.isfinite(z[m])]
        if len(ok) >= 2:
            var[m] = np.std(ok, ddof=1)
    return dict(win_keep=win_keep, cell_keep=cell_keep, motif_keep=motif_keep, sets=sets, rs=rs, d=d, T=T, bg=bg, grid=grid, extremes=extremes,
                O=O, E=E, raw=raw, bg_mean=mean, bg_m2=m2, s=s, deviations=dev, z=z, variability=var,
                annotated=np.array([len(s_) for s_ in sets], np.int64))


def gc_content(seq, start, end):
    """gc of seq[start:end] (bytes), case ignored; 0.5 without an A, C, G or T"""
    s = bytes(seq[start:end]).upper()
    n = [s.count(b) for b in (b"A", b"C", b"G", b"T")]
    return 0.5 if sum(n) == 0 else float(np.float64(n[1] + n[2]) / np.float64(sum(n)))


def base_counts(seq, starts, ends):
    """int64[n, 4]: the A, C, G, T bases of every range, case ignored"""
    out = np.zeros((len(starts), 4), np.int64)
    for i, (s, e) in enumerate(zip(starts, ends)):
        part = bytes(bytearray(seq[int(s):int(e)])).upper()
        out[i] = [part.count(b) for b in (b"A", b"C", b"G", b"T")]
    return out


def file_contents(res, ids, alts, barcodes, B, seed, groups=None):
    """the files of the command from a deviations() result: dict(variability=text, groups=text or None, summary=text, npz=dict of arrays).
    groups: list of (name, list of barcodes), in the order of the table."""
    M_all, kept = len(ids), np.flatnonzero(res["motif_keep"])
    where = {int(k): j for j, k in enumerate(kept)}
    var = [res["variability"][where[k]] if k in where else np.nan for k in range(M_all)]
    wins = [int(res["annotated"][where[k]]) if k in where else 0 for k in range(M_all)]
    order = sorted([k for k in range(M_all) if np.isfinite(var[k])], key=lambda k: (-var[k], k))
    text = "id\talt\twindows\tvariability\trank\n"
    for rank, k in enumerate(order, 1):
        text += "%s\t%s\t%d\t%.6f\t%d\n" % (ids[k], alts[k], wins[k], var[k], rank)
    for k in range(M_all):
        if not np.isfinite(var[k]):
            text += "%s\t%s\t%d\tNA\tNA\n" % (ids[k], alts[k], wins[k])
    kept_bc = [bc for bc, keep in zip(barcodes, res["cell_keep"]) if keep]
    gtext = None
    if groups is not None:
        gtext = "id\t" + "\t".join(name for name, _ in groups) + "\n"
        for k in range(M_all):
            cells = []
            for _, members in groups:
                cols = sorted(kept_bc.index(bc) for bc in members if bc in kept_bc) if k in where else []
                v = [res["z"][where[k], c] for c in cols]
                v = np.array([x for x in v if np.isfinite(x)], np.float64)
                cells.append("%.4f" % (v.sum() / len(v)) if len(v) else "NA")
            gtext += ids[k] + "\t" + "\t".join(cells) + "\n"
    n_w, n_c = len(res["win_keep"]), len(res["cell_keep"])
    summary = ("windows_listed\t%d\nwindows_kept\t%d\nwindows_dropped\t%d\ncells_listed\t%d\ncells_kept\t%d\ncells_dropped\t%d\n"
               "motifs_kept\t%d\nmotifs_dropped\t%d\niterations\t%d\ngc_bins\t%d\nacc_bins\t%d\nsmallest_bin\t%d\nlargest_bin\t%d\nseed\t%d\n"
               % (n_w, res["win_keep"].sum(), n_w - res["win_keep"].sum(), n_c, res["cell_keep"].sum(), n_c - res["cell_keep"].sum(), len(kept),
                  M_all - len(kept), B, res["grid"][0], res["grid"][1], res["extremes"][0], res["extremes"][1], seed))
    N = int(res["cell_keep"].sum())
    dev_all, z_all = np.full((M_all, N), np.nan), np.full((M_all, N), np.nan)
    dev_all[kept], z_all[kept] = res["deviations"], res["z"]
    npz = dict(motifs=np.array([i.encode() for i in ids], dtype="S"), barcodes=np.array(kept_bc, dtype="S"), deviations=dev_all, z=z_all,
               variability=np.array(var, np.float64), windows_annotated=np.array(wins, np.int64))
    return dict(variability=text, groups=gtext, summary=summary, npz=npz)


def npz_bytes(arrays):
    """the .npz the command writes for these arrays: members in the given order, timestamps fixed"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for name, arr in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue())
    return buf.getvalue()


def dense_of(indptr, indices, data, n_cols):
    out = np.zeros((len(indptr) - 1, n_cols), np.int64)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    out[rows, np.asarray(indices, np.int64)] = data
    return out


def csr_of(A):
    """(indptr int64, indices int32, data int32) of the positive entries of a dense matrix"""
    A = np.asarray(A, np.int64)
    r, c = np.nonzero(A)
    indptr = np.zeros(A.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=A.shape[0]), out=indptr[1:])
    return indptr, c.astype(np.int32), A[r, c].astype(np.int32)


def device_standin(indptr, indices, data, n_cells, hit_indptr, hit_indices, n_motifs, bg):
    """what Context.motif_deviations returns, from this module: the host tests inject it for the device call"""
    X = dense_of(indptr, indices, data, n_cells)
    H = dense_of(hit_indptr, hit_indices, np.ones(len(hit_indices), np.int64), n_motifs)
    sets = [np.flatnonzero(H[:, m]) for m in range(n_motifs)]
    full = np.vstack([np.arange(X.shape[0])[None, :], np.asarray(bg, np.int64)])
    O, E = sums(X, sets, full)
    return statistics(O, E, X.sum(axis=0), int(X.sum()))[:3]


def make_case(seed, P=300, N=65, M=5, B=7, big=True, collapse=False):
    """a live matrix at which the kernel can still go wrong: counts from a mix of rates (most cells sparse, a few dense, one window heavy),
    one entry near 2^30 (big), every window and cell with an entry; motif 0 is one window, motif 1 every window (with M == 1: every window
    for an even seed, one window for an odd one), the others random; bg holds arbitrary windows, or one window for all (collapse: the
    window of the large entry, so that a counter passes 2^32).  -> dict(X dense, H dense, bg int32[B, P], csr, hits)"""
    rng = np.random.default_rng(seed)
    rate = np.where(rng.random(N) < 0.15, 3.0, 0.08)[None, :] * np.where(rng.random(P) < 0.02, 20.0, 1.0)[:, None]
    X = rng.poisson(rate).astype(np.int64)
    X[np.arange(P), rng.integers(0, N, P)] += 1                       # no empty window
    X[rng.integers(0, P, N), np.arange(N)] += 1                       # no empty cell
    heavy = int(rng.integers(0, P))
    if big:
        X[heavy, int(rng.integers(0, N))] = (1 << 30) - int(rng.integers(0, 1000))
    H = np.zeros((P, M), np.int64)
    kinds = (["all", "one"][seed % 2:][:1] if M == 1 else ["one", "all"] + ["random"] * (M - 2))
    for m, kind in enumerate(kinds):
        if kind == "one":
            H[int(rng.integers(0, P)), m] = 1
        elif kind == "all":
            H[:, m] = 1
        else:
            H[rng.random(P) < rng.uniform(0.02, 0.4), m] = 1
            H[int(rng.integers(0, P)), m] = 2
    bg = np.full((B, P), heavy, np.int32) if collapse else rng.integers(0, P, (B, P)).astype(np.int32)
    hp, hx, _ = csr_of(H)
    return dict(X=X, H=H, bg=bg, csr=csr_of(X), hits=(hp, hx), sets=[np.flatnonzero(H[:, m]) for m in range(M)], heavy=heavy)


def make_arm_case(seed, P, N, B, sizes, density, full=0.01, planted=None, to_planted=False):
    """a live matrix made to select one arm of the kernel (tests/test_gpu_deviations_arms.py): every entry present with probability
    `density`, a share `full` of the windows with an entry in every cell, every window and cell left empty patched with one entry, counts
    of 1 .. 8; planted: the value of one entry put at a random place (case["heavy"], case["heavy_cell"]).  Motif k is the first sizes[k]
    windows of a random permutation, sorted.  bg holds arbitrary windows; to_planted: set 1 maps every window to the planted entry's
    window.  -> the dict of make_case()"""
    rng = np.random.default_rng(seed)
    X = np.where(rng.random((P, N)) < density, rng.integers(1, 9, (P, N)), 0).astype(np.int64)
    rows = rng.choice(P, int(round(full * P)), replace=False)
    X[rows] = rng.integers(1, 9, (len(rows), N))
    empty = np.flatnonzero(X.sum(axis=1) == 0)
    X[empty, rng.integers(0, N, len(empty))] = rng.integers(1, 9, len(empty))
    empty = np.flatnonzero(X.sum(axis=0) == 0)
    X[rng.integers(0, P, len(empty)), empty] = rng.integers(1, 9, len(empty))
    heavy, heavy_cell = int(rng.integers(0, P)), int(rng.integers(0, N))
    if planted is not None:
        X[heavy, heavy_cell] = planted
    sets = [np.sort(rng.permutation(P)[:k]) for k in sizes]
    H = np.zeros((P, len(sizes)), np.int64)
    for m, s in enumerate(sets):
        H[s, m] = 1
    bg = rng.integers(0, P, (B, P)).astype(np.int32)
    if to_planted:
        bg[0] = heavy
    hp, hx, _ = csr_of(H)
    return dict(X=X, H=H, bg=bg, csr=csr_of(X), hits=(hp, hx), sets=sets, heavy=heavy, heavy_cell=heavy_cell)


def reference_of(case):
    """(O, E, raw, bg_mean, bg_m2, s) of a make_case() or make_arm_case() result"""
    full = np.vstack([np.arange(case["X"].shape[0])[None, :], case["bg"].astype(np.int64)])
    O, E = sums(case["X"], case["sets"], full)
    return (O, E) + statistics(O, E, case["X"].sum(axis=0), int(case["X"].sum()))


# ---- files for the command's tests ----
def regions(n, width=40):
    chrom = ["chrA" if i % 3 else "chrB" for i in range(n)]
    start = np.array([(i * 17) % 400 for i in range(n)], np.int64)
    return chrom, start, start + width


def write_inputs(base, X, H, barcodes, ids, alts, fmt_x, fmt_h, regions_x=None, regions_h=None):
    """what `cellcounts --format fmt_x` and `motifs --format fmt_h` write, as far as `deviations` reads them"""
    from nucleoatac_amd.pyatac.get_cellcounts import mtx_text
    chrom, start, end = regions_x or regions(len(X))
    out = []
    for name, A, fmt, side, (c, s, e) in (("cellcounts", X, fmt_x, "barcodes", (chrom, start, end)),
                                          ("motifs", H, fmt_h, "names", regions_h or (chrom, start, end))):
        ip, ix, da = csr_of(A)
        if fmt == "npz":
            extra = dict(barcodes=np.array(barcodes, dtype="S")) if name == "cellcounts" else \
                dict(motifs=np.array(ids, dtype="S"), alts=np.array(alts, dtype="U"))
            np.savez_compressed("%s.%s.npz" % (base, name), indptr=ip, indices=ix, data=da, shape=np.array(A.shape, np.int64),
                                region_chrom=np.array(c, dtype="U"), region_start=s, region_end=e, **extra)
            out.append("%s.%s.npz" % (base, name))
            continue
        with gzip.open("%s.%s.mtx.gz" % (base, name), "wb") as f:
            f.write(mtx_text(ip, ix, da, A.shape[1]))
        with open("%s.%s.%s.tsv" % (base, name, side), "wb") as f:
            if name == "cellcounts":
                f.write(b"".join(b + b"\n" for b in barcodes))
            else:
                f.write("".join("%s\t%s\n" % p for p in zip(ids, alts)).encode())
        with open("%s.%s.regions.bed" % (base, name), "w") as f:
            f.write("".join("%s\t%d\t%d\n" % r for r in zip(c, s.tolist(), e.tolist())))
        out.append("%s.%s.mtx.gz" % (base, name))
    return out


def write_fasta(path, seed=5):
    rng = np.random.default_rng(seed)
    seqs = {}
    with open(path, "w") as f:
        for name in ("chrA", "chrB"):
            p = rng.uniform(0.1, 0.4, 10).repeat(50)
            s = np.where(rng.random(500) < p, rng.choice(list(b"CG"), 500), rng.choice(list(b"AT"), 500)).astype(np.uint8)
            s[100:110] = ord("N")
            seqs[name] = s
            f.write(">%s\n%s\n" % (name, s.tobytes().decode()))
    return seqs
