"""GPU: the drivers' fallbacks for a chunk with more local maxima than the register peak kernels keep (PEAK_MAX = 2,048; status
value 2): Occupancy.occ_batch and NucleosomeCalling.nuc_batch redo such a chunk on the host, `nucleoatac occ`
(run_occ.peaks_and_dists) and `nucleoatac nuc` (run_nuc.batch_calls_start / _finish) merge the redone chunk back in chunk order.

The input is realistic: a 15,200-base region densely covered by 150-190 bp fragments.  Its occupancy is saturated at 1.0, so the
jittered track has about one maximum in three bases (~5,000 at order 1, occupancy peaks); norm + smoothed at --redundant_sep 2
(order 1) has ~2,150 maxima of at least 0 inside the boundary bands without a FASTA (counted with the oracle on the CPU).  With
the Human PWM bias of a random sequence the same chunk has only ~1,800 (no overflow), so the nucleosome tests run without a FASTA,
as `nucleoatac nuc` allows.  15,200 bases keep the batch on natac_peaks_chunk_reg<15, 1024>.  Every test asserts that the chunk
really overflowed, so the path stays covered."""
import gzip

import numpy as np
import pytest

from helpers import call_peaks_stable, golden

pytestmark = pytest.mark.gpu

CHROM_LEN = 110000
SAT = (40000, 55200)                   # the saturated chunk (15,200 bases)
ORDINARY = [(6000, 9000), (20000, 25000), (62000, 64500), (75000, 79000)]
LONG = (7000, 24000)                   # 17,000 bases: pushes a batch onto the segmented kernel (global lists)
FAR = (86000, 103000)                  # the same for the CLI runs, apart from every other region
MIN_OCC, OCC_SEP, FLANK = 0.1, 120, 60
NONRED_SEP, RED_SEP = 120, 2           # order = redundant_sep // 2 = 1


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """synthetic chrS: nucleosome-like fragments at 0.35 per base everywhere, 3 per base of 150-190 bp over the saturated region"""
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    from nucleoatac_amd.pyatac.seq import FastaStore
    from nucleoatac_amd.synth import synth_centres, synth_sizes
    rng = np.random.default_rng(29)
    nf = int(CHROM_LEN * 0.35)
    n = synth_sizes(rng, nf).astype(np.int64)
    c = synth_centres(rng, nf, CHROM_LEN - 1600) + 800
    out = (c < SAT[0] - 300) | (c >= SAT[1] + 300)           # no sub-nucleosomal fragments there: occupancy saturates at 1.0
    n, c = n[out], c[out]
    ns = 3 * (SAT[1] - SAT[0] + 600)
    n = np.concatenate([n, rng.integers(150, 191, size=ns)])
    c = np.concatenate([c, rng.integers(SAT[0] - 300, SAT[1] + 300, size=ns)])
    l = c - (n - 1) // 2
    o = np.argsort(l, kind="stable")
    l, n = l[o], n[o]
    seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=CHROM_LEN)
    frags = FragmentStore(["chrS"], [CHROM_LEN], {"chrS": l - 4}, {"chrS": n + 8})
    d = tmp_path_factory.mktemp("overflow")
    bam = str(d / "sat.npz")
    frags.save_npz(bam)
    fa = str(d / "sat.fa")
    with open(fa, "w") as f:
        f.write(">chrS\n")
        s = seq.tobytes().decode()
        for i in range(0, len(s), 60):
            f.write(s[i:i + 60] + "\n")
    return dict(frags=frags, fasta=FastaStore({"chrS": seq.copy()}), bam=bam, fa=fa, dir=d)


def _params(genome):
    from nucleoatac_amd.nucleoatac.NucleosomeCalling import NucParameters
    from nucleoatac_amd.nucleoatac.Occupancy import FragmentMixDistribution, OccupancyParameters
    from nucleoatac_amd.pyatac.fragmentsizes import FragmentSizes
    from nucleoatac_amd.pyatac.VMat import VMat
    par = golden("params_example")
    fd = FragmentMixDistribution(0, 251)
    fd.fragmentsizes = FragmentSizes(0, 251, vals=par["sizes"])
    fd.nuc_fit = FragmentSizes(0, 251, vals=par["nuc_probs"])
    fd.nfr_fit = FragmentSizes(0, 251, vals=par["nfr_probs"])
    op = OccupancyParameters(fd, 251, genome["fasta"], "Human", sep=OCC_SEP, min_occ=MIN_OCC, flank=FLANK, bam=genome["frags"],
                             ci=0.9, step=5)
    op.fasta = None
    npar = NucParameters(vmat=VMat(par["vmat"], int(par["vlower"]), int(par["vupper"])),
                         fragmentsizes=FragmentSizes(0, 251, vals=par["sizes"]), bam=genome["frags"], fasta=None, pwm="Human",
                         occ_track=None, sd=10, nonredundant_sep=NONRED_SEP, redundant_sep=RED_SEP, min_z=3, min_lr=0, atac=True)
    return op, npar


def _chunks(where):
    """the saturated chunk first, in the middle or last among ordinary (shorter) chunks"""
    from nucleoatac_amd.pyatac.chunk import Chunk
    ords = [Chunk("chrS", a, b) for a, b in ORDINARY[:3]]
    sat = Chunk("chrS", *SAT)
    k = {"first": 0, "middle": 1, "last": 3}[where]
    return ords[:k] + [sat] + ords[k:], k


def _occ_expected(op, chunks, k):
    """OccChunk.callPeaks + getNucDist of chunk k restated on the host from the device's own tracks (as tests/fuzz/fuzz_parity.py):
    stable call_peaks, the OccPeak values, the occ_lower > min_occ / reads > 0 filter, the nuc_dist histogram.  Also asserts that
    the device's peak search flagged chunk k (and no other) as overflowing."""
    from nucleoatac_amd.pipeline import BatchRunner, pack
    from nucleoatac_amd import get_context
    ctx = get_context()
    op.occ_calc_params.install(ctx, step=op.step, flank=op.flank)
    pk = pack(chunks, op.bam, op.fasta, op.chrs, None, window=op.window, upper=op.upper)
    run = BatchRunner(pk, ctx)
    try:
        res = run.occ()
        run.batch.run_occ_peaks(min_occ=op.min_occ, sep=op.sep)
        st = run.batch.status()
    finally:
        run.close()
    assert [int(s) & 2 for s in st] == [2 if i == k else 0 for i in range(len(chunks))], st
    occ, lo, up, cov = (res[n][k] for n in ("smoothed_vals", "smoothed_lower", "smoothed_upper", "cov"))
    pks = np.asarray(call_peaks_stable(occ.copy(), sep=op.sep, min_signal=op.min_occ, boundary=op.sep // 2, order=1), np.int64)
    assert len(pks) > 0
    keep = (lo[pks] > op.min_occ) & (cov[pks] > 0)
    l, n = pk.chunk_frags(k)
    cen = l + (n - 1) // 2
    nd = np.zeros(op.upper)
    for p in pks[keep]:
        sel = (cen >= p - op.flank) & (cen <= p + op.flank) & (n >= 0) & (n < op.upper)
        h = np.bincount(n[sel], minlength=op.upper)[:op.upper].astype(np.float64)
        nd += h / h.sum()
    vals = {int(p): (occ[p], lo[p], up[p], cov[p]) for p in pks[keep]}
    return vals, nd


def _occ_objects_equal(a, b, nd_exact=True):
    assert sorted(a.peaks) == sorted(b.peaks)
    for p in a.peaks:
        x, y = a.peaks[p], b.peaks[p]
        assert (x.start, x.occ, x.occ_lower, x.occ_upper, x.reads) == (y.start, y.occ, y.occ_lower, y.occ_upper, y.reads), p
    if nd_exact:
        assert np.array_equal(a.getNucDist(), b.getNucDist())
    else:
        np.testing.assert_allclose(a.getNucDist(), b.getNucDist(), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_occ_batch_overflow_fallback(genome, where):
    """occ_batch: the flagged chunk's peaks, OccPeak values, filter and nuc_dist == the host restatement; the other chunks ==
    occ_batch of those chunks alone; the saturated chunk in a batch on the segmented kernel gives the same objects"""
    from nucleoatac_amd.nucleoatac.Occupancy import occ_batch
    from nucleoatac_amd.pyatac.chunk import Chunk
    op, _ = _params(genome)
    chunks, k = _chunks(where)
    vals, nd = _occ_expected(op, chunks, k)
    ocs = occ_batch(chunks, op)
    oc = ocs[k]
    assert sorted(oc.peaks) == sorted(vals) and len(vals) > 50
    for p, (o, lo, up, rd) in vals.items():
        x = oc.peaks[p]
        assert x.start == p + SAT[0] and (x.occ, x.occ_lower, x.occ_upper, x.reads) == (o, lo, up, rd), p
    np.testing.assert_allclose(oc.getNucDist(), nd, rtol=1e-12, atol=1e-15)
    alone = occ_batch([c for i, c in enumerate(chunks) if i != k], op)
    for a, b in zip([x for i, x in enumerate(ocs) if i != k], alone):
        _occ_objects_equal(a, b)
    seg = occ_batch([chunks[k], Chunk("chrS", *LONG)], op)       # maxL 17,000: global lists, no overflow, device nuc_dist
    _occ_objects_equal(oc, seg[0], nd_exact=False)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_nuc_batch_overflow_fallback(genome, where):
    """nuc_batch: the flagged chunk's candidates == stable call_peaks on the device's norm + smoothed, lr / z == natac_run_candidates
    there, and its calls (nonredundant / redundant, every value) == the same chunk in a batch on the segmented kernel"""
    from nucleoatac_amd.nucleoatac.NucleosomeCalling import nuc_batch
    from nucleoatac_amd.pipeline import BatchRunner, pack
    from nucleoatac_amd.pyatac.chunk import Chunk
    from nucleoatac_amd import get_context
    _, npar = _params(genome)
    chunks, k = _chunks(where)
    ctx = get_context()
    npar.install(ctx)
    run = BatchRunner(pack(chunks, npar.bam, None, npar.chrs, npar.pwm, atac=npar.atac, window=npar.window, upper=npar.upper), ctx)
    try:
        res = run.nuc(npar.smooth_sd)
        run.batch.run_peaks(min_signal=0, sep=RED_SEP, boundary=NONRED_SEP // 2, order=RED_SEP // 2)
        st = run.batch.status()
        assert [int(s) & 2 for s in st] == [2 if i == k else 0 for i in range(len(chunks))], st
        cands = np.asarray(call_peaks_stable(res["norm_signal"][k] + res["smoothed"][k], min_signal=0, sep=RED_SEP,
                                             boundary=NONRED_SEP // 2, order=RED_SEP // 2), np.int32)
        lr, _var, z = run.batch.run_candidates(np.full(len(cands), k, np.int32), cands)
    finally:
        run.close()
    ncs = nuc_batch(chunks, npar)
    nc = ncs[k]
    assert np.array_equal(np.asarray(nc._cands, np.int64), cands.astype(np.int64)) and len(cands) > 2048
    at = {int(p): i for i, p in enumerate(cands)}
    assert len(nc.nuc_collection) > 0
    for p, nu in nc.nuc_collection.items():
        assert (nu.lr, nu.z) == (lr[at[int(p)]], z[at[int(p)]]), p
    seg = nuc_batch([chunks[k], Chunk("chrS", *LONG)], npar)[0]
    assert sorted(nc.nonredundant) == sorted(seg.nonredundant) and sorted(nc.redundant) == sorted(seg.redundant)
    assert len(nc.nonredundant) > 0 and len(nc.redundant) > 0
    for p in nc.nuc_collection:
        a, b = nc.nuc_collection[p], seg.nuc_collection[p]
        va = np.array([a.start, a.z, a.lr, a.norm_signal, a.nuc_signal, a.nuc_cov, a.nfr_cov, a.fuzz], np.float64)
        vb = np.array([b.start, b.z, b.lr, b.norm_signal, b.nuc_signal, b.nuc_cov, b.nfr_cov, b.fuzz], np.float64)
        assert np.array_equal(va, vb, equal_nan=True), p


# ---- the CLI: one rank, a few chunks ------------------------------------------------------------------------------------------

def _bed(path, regions):
    with open(path, "w") as f:       # the drivers slop by nuc_sep / 2 = 60 and merge: give the un-slopped regions
        for a, b in regions:
            f.write("chrS\t%d\t%d\n" % (a + 60, b - 60))
    return path


def _rows(path):
    with gzip.open(path, "rt") as fh:
        return [l for l in fh.read().split("\n") if l]


def _split(rows, regions):
    """rows by region; every row lies in one region"""
    out = {r: [] for r in regions}
    for row in rows:
        p = int(row.split("\t")[1])
        hit = [r for r in regions if r[0] <= p < r[1]]
        assert len(hit) == 1, row
        out[hit[0]].append(row)
    return out


def _assert_chunk_order(rows):
    pos = [int(r.split("\t")[1]) for r in rows]
    assert pos == sorted(pos) and len(set(pos)) == len(pos), "rows out of chunk order or duplicated"


def _cli_files(genome):
    from nucleoatac_amd.pyatac.fragmentsizes import FragmentSizes
    par = golden("params_example")
    d = genome["dir"]
    sizes = str(d / "sizes.txt")
    FragmentSizes(0, 251, vals=par["sizes"]).save(sizes)
    vm = str(d / "v.npz")
    np.savez(vm, vmat=par["vmat"], vlower=par["vlower"], vupper=par["vupper"])
    return sizes, vm


def test_cli_occ_overflow(genome, monkeypatch):
    """`nucleoatac occ` on a BED with the saturated region in the middle: occpeaks rows in chunk order without duplicates, the
    saturated chunk's rows == those of a run that keeps it on the device (a 17-kb region in the BED: segmented kernel), every other
    chunk's rows byte-identical to a run without the saturated region, and nuc_dist == that run's per-chunk sum with the saturated
    chunk's host getNucDist inserted at its place, summed in chunk order (shard.ordered_sum)"""
    from nucleoatac_amd.nucleoatac import run_occ
    from nucleoatac_amd.nucleoatac.cli import main
    from nucleoatac_amd.pyatac.tracks import _py2_float_str
    sizes, _ = _cli_files(genome)
    d = genome["dir"]
    regs = [ORDINARY[0], ORDINARY[1], SAT, ORDINARY[2], ORDINARY[3]]
    far = FAR
    rec = {"dists": [], "redo": []}
    real_sum, real_occ_batch = run_occ.ordered_sum, run_occ.occ_batch

    def spy_sum(v):
        rec["dists"].append([np.array(x) for x in v])
        return real_sum(v)

    def spy_occ_batch(chunks, params, *a, **kw):
        r = real_occ_batch(chunks, params, *a, **kw)
        rec["redo"].append([(c.start, c.end, o.getNucDist().copy()) for c, o in zip(chunks, r)])
        return r

    monkeypatch.setattr(run_occ, "ordered_sum", spy_sum)
    monkeypatch.setattr(run_occ, "occ_batch", spy_occ_batch)
    outs = {}
    for name, rr in (("main", regs), ("nosat", [r for r in regs if r != SAT]), ("seg", regs + [far])):
        out = str(d / ("occ_" + name))
        rec["redo"].append(name)
        main(["occ", "--bed", _bed(str(d / (name + ".bed")), rr), "--bam", genome["bam"], "--fasta", genome["fa"], "--out", out,
              "--sizes", sizes])
        outs[name] = (out, _rows(out + ".occpeaks.bed.gz"), rec["dists"][-1])
    # the fallback ran for the saturated chunk only, and only in the run on the register kernel
    calls = {}
    for x in rec["redo"]:
        if isinstance(x, str):
            cur = calls.setdefault(x, [])
        else:
            cur.extend(x)
    assert [(a, b) for a, b, _ in calls["main"]] == [SAT] and calls["nosat"] == [] and calls["seg"] == []
    main_rows, nosat_rows, seg_rows = outs["main"][1], outs["nosat"][1], outs["seg"][1]
    _assert_chunk_order(main_rows)
    by_main, by_nosat, by_seg = _split(main_rows, regs), _split(nosat_rows, regs), _split(seg_rows, regs + [far])
    assert len(by_main[SAT]) > 50 and by_main[SAT] == by_seg[SAT]
    for r in regs:
        if r != SAT:
            assert by_main[r] == by_nosat[r] and by_main[r] == by_seg[r], r
    dm, dn, ds = outs["main"][2], outs["nosat"][2], outs["seg"][2]
    k = regs.index(SAT)
    assert len(dm) == len(regs) and len(dn) == len(regs) - 1
    assert all(np.array_equal(a, b) for a, b in zip(dm[:k] + dm[k + 1:], dn))
    host_nd = calls["main"][0][2]
    assert np.array_equal(dm[k], host_nd)
    np.testing.assert_allclose(dm[k], ds[k], rtol=1e-12, atol=1e-15)      # the device's histogram of the same peaks
    want = dn[0].copy()
    for v in dn[1:k] + [host_nd] + dn[k:]:
        want = want + v
    with open(outs["main"][0] + ".nuc_dist.txt") as fh:
        got = fh.read().strip().split("\n")[-1].split("\t")
    assert got == [_py2_float_str(float(x)) for x in want]


def test_cli_nuc_overflow(genome, monkeypatch):
    """`nucleoatac nuc --redundant_sep 2` (no FASTA: see the module docstring) on a BED with the saturated region in the middle: nucpos / nucpos.redundant rows in chunk
    order without duplicates (the truncated device rows of the saturated chunk are dropped, its host rows inserted once), its rows
    == a run that keeps it on the device (segmented kernel), every other chunk's rows byte-identical to a run without it"""
    from nucleoatac_amd.nucleoatac import run_nuc
    from nucleoatac_amd.nucleoatac.cli import main
    sizes, vm = _cli_files(genome)
    d = genome["dir"]
    regs = [ORDINARY[0], ORDINARY[1], SAT, ORDINARY[2], ORDINARY[3]]
    far = FAR
    redo = []
    real = run_nuc.nuc_batch

    def spy(chunks, params, *a, **kw):
        redo.append([(c.start, c.end) for c in chunks])
        return real(chunks, params, *a, **kw)

    monkeypatch.setattr(run_nuc, "nuc_batch", spy)
    rows = {}
    for name, rr in (("main", regs), ("nosat", [r for r in regs if r != SAT]), ("seg", regs + [far])):
        out = str(d / ("nuc_" + name))
        n0 = len(redo)
        main(["nuc", "--bed", _bed(str(d / ("n" + name + ".bed")), rr), "--bam", genome["bam"], "--out", out, "--sizes", sizes,
              "--vmat", vm, "--redundant_sep", str(RED_SEP)])
        rows[name] = {f: _rows(out + "." + f + ".bed.gz") for f in ("nucpos", "nucpos.redundant")}
        rows[name]["redo"] = redo[n0:]
    assert rows["main"]["redo"] == [[SAT]] and rows["nosat"]["redo"] == [] and rows["seg"]["redo"] == []
    for f in ("nucpos", "nucpos.redundant"):
        _assert_chunk_order(rows["main"][f])
        bm, bn, bs = _split(rows["main"][f], regs), _split(rows["nosat"][f], regs), _split(rows["seg"][f], regs + [far])
        assert len(bm[SAT]) > 0 and bm[SAT] == bs[SAT], f
        for r in regs:
            if r != SAT:
                assert bm[r] == bn[r] and bm[r] == bs[r], (f, r)
