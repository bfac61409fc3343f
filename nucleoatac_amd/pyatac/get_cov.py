"""`pyatac cov`: the coverage of fragment centres over a flat window (the reference's pyatac/get_cov.py).

The reference builds a FragmentMat2D of [start - W//2, end + W//2) for every region, sums its rows and smooths them with a flat window
of W taps (W + 1 when W is even), then multiplies by scale / float(W) (get_cov.py:21-37, tracks.py:209-222).  natac_run_center_cov
counts the same centres in an LDS histogram and takes each window sum from an integer prefix, so every value is the same exact count
times the same fp64 factor: bit-identical.
"""
from .trackfiles import default_out, track_regions, write_track_file


def get_cov(args, timing=None):
    """writes <out>.cov.bedgraph.gz and its .tbi (get_cov.py:40-76); raises trackfiles.MissingChromosomeError (no file written) for a
    BED region on a chromosome the BAM lacks"""
    from .. import _lib as L
    args.out = default_out(args)
    W = int(args.window)
    if W < 1:
        raise ValueError("--window must be at least 1 (got %d)" % W)
    mult = args.scale / float(W)
    chunks = track_regions(args.bam, args.bed)

    def run(b):
        b.run_center_cov(W, mult, args.lower, args.upper)
        return L.T_CENTER_COV
    return write_track_file(args.out + ".cov.bedgraph.gz", chunks, args.bam, run, W // 2, args.lower, args.upper, args.atac,
                            timing=timing)
