"""`pyatac sizes`: the fragment-size distribution of a BAM (the reference's pyatac/get_sizes.py) -- the `--sizes` input of
`nucleoatac occ` / `nuc`.  The histogram is natac_fragment_sizes (FragmentSizes.calculateSizes); no plots are made."""
import os

from .chunk import ChunkList
from .fragmentsizes import FragmentSizes


def get_sizes(args):
    """writes <out>.fragmentsizes.txt (get_sizes.py:16-27): all fragments, or with --bed those centred in the merged regions"""
    if args.out is None:
        args.out = ".".join(os.path.basename(args.bam).split(".")[0:-1])
    sizes = FragmentSizes(lower=args.lower, upper=args.upper, atac=args.atac)
    if args.bed:
        chunks = ChunkList.read(args.bed)
        chunks.merge()
        sizes.calculateSizes(args.bam, chunks)
    else:
        sizes.calculateSizes(args.bam)
    sizes.save(args.out + ".fragmentsizes.txt")
    return sizes
