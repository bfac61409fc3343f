"""`pyatac ins`: the Tn5 insertion track of a BAM, raw or Gaussian-smoothed (the reference's pyatac/get_ins.py).

Without --smooth (or with 0) every region's track is getInsertions (natac_run_ins, fragments.pyx:43-67), written as floats like the
reference's.  With --smooth S the insertions of [start - S//2, end + S//2) are smoothed by utils.smooth(..., window="gaussian",
mode="valid", norm=True) (get_ins.py:20-32, utils.py:23-52) in natac_run_ins_smooth: an even S gets one more tap, the window and its
normaliser come from scipy on the host, each value is an fp64 window sum divided by that normaliser.
"""
from .trackfiles import default_out, gaussian_window, track_regions, write_track_file


def get_ins(args, timing=None):
    """writes <out>.ins.bedgraph.gz and its .tbi (get_ins.py:60-85); raises trackfiles.MissingChromosomeError (no file written) for a
    BED region on a chromosome the BAM lacks"""
    from .. import _lib as L
    args.out = default_out(args)
    smooth = int(args.smooth or 0)
    if smooth < 0:
        raise ValueError("--smooth must not be negative (got %d)" % smooth)
    chunks = track_regions(args.bam, args.bed)
    if smooth:
        w, wsum = gaussian_window(smooth)

        def run(b):
            b.run_ins_smooth(w, args.lower, args.upper, wsum)
            return L.T_INS_SMOOTH
    else:
        def run(b):
            b.run_ins(args.lower, args.upper)
            return L.T_INS
    return write_track_file(args.out + ".ins.bedgraph.gz", chunks, args.bam, run, smooth // 2, args.lower, args.upper, args.atac,
                            timing=timing)
