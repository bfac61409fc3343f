"""`pyatac pwm | sizes` command line with the reference's flag names and defaults (pyatac/cli.py:111-173).  These are the two pyatac
tools whose outputs feed `nucleoatac occ` / `nuc` (--pwm, --sizes); the other pyatac tools are not part of this package."""
import argparse
import sys


def add_pwm_parser(sub):
    p = sub.add_parser("pwm", help="pyatac function-- get nucleotide content around insertion sites")
    p.add_argument("--fasta", required=True, help="Accepts fasta file")
    p.add_argument("--bam", required=True, help="Reads around which to get nucleotide freq (BAM or a FragmentStore .npz)")
    p.add_argument("--bed", help="Regions from which to use reads")
    p.add_argument("--dinucleotide", action="store_true", default=False, help="accepted for compatibility; ignored, like the reference")
    p.add_argument("--flank", type=int, default=10, help="Bases away from insertion site to get frequencies for. Default is 10")
    p.add_argument("--lower", type=int, default=0, help="lower limit on insert size. default is 0")
    p.add_argument("--upper", type=int, default=2000, help="upper limit on insert size. default is 2000")
    p.add_argument("--not_atac", dest="atac", action="store_false", default=True, help="Don't use atac offsets")
    p.add_argument("--no_sym", dest="sym", action="store_false", default=True, help="Don't symmetrize PWM")
    p.add_argument("--out", help="Basename for output")
    p.add_argument("--cores", type=int, default=1, help="accepted for compatibility; the GPU replaces the pool")


def add_sizes_parser(sub):
    p = sub.add_parser("sizes", help="pyatac function-- compute fragment size distribution")
    p.add_argument("--bam", required=True, help="Aligned reads (BAM or a FragmentStore .npz)")
    p.add_argument("--bed", help="Only compute size distribution for fragment centered within regions in bed file")
    p.add_argument("--out", help="Basename for output")
    p.add_argument("--not_atac", dest="atac", action="store_false", default=True, help="Don't use atac offsets")
    p.add_argument("--lower", type=int, default=0, help="lower limit on insert size. Default is 0")
    p.add_argument("--upper", type=int, default=500, help="upper limit on insert size. Default is 500")
    p.add_argument("--no_plot", action="store_true", default=False, help="accepted for compatibility; plots are never made")


def pyatac_parser():
    from .. import __version__
    parser = argparse.ArgumentParser(prog="pyatac", description="pyatac: fit the Tn5 PWM and the fragment-size distribution")
    parser.add_argument("--version", action="version", version="%(prog)s " + __version__)
    sub = parser.add_subparsers(dest="call")
    sub.required = True
    add_pwm_parser(sub)
    add_sizes_parser(sub)
    return parser


def pyatac_main(args):
    if args.call == "pwm":
        from .get_pwm import PWMFitError, get_pwm
        print("---------Making PWM from bam---------------------------------------")
        try:
            get_pwm(args)
        except PWMFitError as e:
            sys.stderr.write("pyatac pwm: %s\n" % e)
            return 1
    elif args.call == "sizes":
        from .get_sizes import get_sizes
        print("---------Getting fragment sizes---------------------------------------")
        print("plots are not produced: only the .fragmentsizes.txt file is written")
        get_sizes(args)
    return 0


def main(argv=None):
    return pyatac_main(pyatac_parser().parse_args(argv))


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
