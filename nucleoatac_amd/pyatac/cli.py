"""`pyatac pwm | sizes | ins | cov | bias | counts | nucleotide | signal | cells | cellqc | split | cellcounts | doublets | cluster | deviations | markers | coaccess | genescores | peaks | motifs` command line with the reference's flag names and defaults
(pyatac/cli.py:90-193, 270-352).  `pwm` and `sizes` make the --pwm and --sizes inputs of `nucleoatac occ` / `nuc`; `ins` and `cov`
write the per-base insertion and fragment-centre coverage tracks, `bias` the per-base log Tn5 preference of a FASTA under a PWM;
`counts` gives the fragment count of every BED window, `nucleotide` the mono- or dinucleotide frequency around a set of sites
(for one, the nucpos.bed.gz of `nucleoatac nuc`) and `signal` the values of an indexed bedGraph track (any of the tracks written here)
around such sites, per site and summed.  `split` is this package's own: it splits a single-cell fragment file by cell barcode into one
store per cell group (a cluster, a sample, a whitelist) in one pass, each written as .npz or as a fragment file that every command above
takes through --bam.  `cellcounts` is this package's own too: the cell-by-window count matrix of a single-cell fragment file (rows the BED
windows, columns the barcodes of a table), sparse, as MatrixMarket text or .npz.  `cells`, this package's own as well, comes before both: it
discovers the barcodes of a single-cell fragment file with per-cell fragment counts and writes the table of those that pass the user's
thresholds, which `split --groups` and `cellcounts --cells` take unchanged.  `cellqc`, this package's own too, stands between them: for
the barcodes of such a table it gives per-cell TSS enrichment (insertions around a BED of transcription start sites, with the aggregate
profile) and FRiP (the fraction of a cell's fragments in a BED of peaks), and writes the table of the cells that pass the user's thresholds
on those.  `peaks`, this package's own as well, makes the peak set the other commands take (`counts --bed`, `cellqc --peaks`, `cellcounts
--bed`, `nucleoatac run --bed`) from nothing but the fragments: regions whose insertion pileup is improbable at the genome-wide and at
two local rates, as a narrowPeak file and, with --fixed_width, as disjoint windows of one width; run per cell group behind `split`, it is
the last link before `nucleoatac run`.  `cluster`, this package's own too, makes the group column `split --groups` wants from the matrix
`cellcounts` wrote: TF-IDF weighting, a truncated SVD of the weighted matrix on the GPU (LSI), the depth-tracking components removed and
k-means with a given number of clusters.  `doublets`, this package's own as well, comes before it: it simulates doublets by adding two
cells' counts, puts them into the same LSI space, scores every cell by the share of simulated doublets among its nearest neighbours (an
exact search on the GPU) and writes the table of the cells to keep, which `cellcounts --cells` takes unchanged.  The single-cell chain is
`cells` -> `cellqc` -> `peaks` (whole file) -> `cellcounts` -> `doublets` -> `cellcounts --cells` ->
`cluster` -> `deviations` / `markers` / `coaccess` / `genescores` / `split` -> `peaks` per group -> `nucleoatac run`, with no outside tool.  `motifs`, this package's own as well, makes the
sites that `signal --bed`, `nucleotide --bed` and `cellqc --tss` aggregate around: it scans the FASTA, or the windows of a BED file, for
the motifs of a MEME or JASPAR file on the GPU and writes the sites and the window-by-motif match matrix.  `deviations`, this package's
own too, joins that matrix with the `cellcounts` matrix: per-cell motif accessibility deviations and z-scores against background window
sets matched in GC content and accessibility, summed on the GPU, with a variability ranking of the motifs and, with the table `cluster`
writes, the mean z-score per cluster.  `markers`, this package's own as well, answers which windows distinguish a cluster from the rest:
a Wilcoxon rank-sum test of depth-normalised accessibility, one group of that table against all other cells, for every window and group,
the ranking done on the GPU in exact integers, with Benjamini-Hochberg q-values, a marker table and one BED file per group that the
commands above take through --bed.  `coaccess`, this package's own too, answers which windows open and close together: the Pearson
correlation over the cells (or, with --aggregate, over the clusters of that table as metacells) of every two windows of a chromosome
within --max_distance of each other, the sparse row intersections done on the GPU in exact integers, with a t-test, Benjamini-Hochberg
q-values and a BEDPE file of links.  `genescores`, this package's own as well, is the bridge from windows to genes: per gene and cell
the sum over the cell's insertions around the gene of an integer weight that falls with the distance to the gene body, the window capped
at the neighbouring genes, summed on the GPU in exact integers and written in the `cellcounts` layout, so that `markers --counts
BASE.genescores.npz` names the genes that distinguish a cluster.  The other pyatac tools (vplot, bias_vplot) are not part of
this package."""
import argparse
import sys


def add_pwm_parser(sub):
    p = sub.add_parser("pwm", help="pyatac function-- get nucleotide content around insertion sites")
    p.add_argument("--fasta", required=True, help="Accepts fasta file")
    p.add_argument("--bam", required=True, help="Reads around which to get nucleotide freq (BAM, fragment file or FragmentStore .npz)")
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
    p.add_argument("--bam", required=True, help="Aligned reads (BAM, fragment file or FragmentStore .npz)")
    p.add_argument("--bed", help="Only compute size distribution for fragment centered within regions in bed file")
    p.add_argument("--out", help="Basename for output")
    p.add_argument("--not_atac", dest="atac", action="store_false", default=True, help="Don't use atac offsets")
    p.add_argument("--lower", type=int, default=0, help="lower limit on insert size. Default is 0")
    p.add_argument("--upper", type=int, default=500, help="upper limit on insert size. Default is 500")
    p.add_argument("--no_plot", action="store_true", default=False, help="accepted for compatibility; plots are never made")


def _add_track_options(p):
    p.add_argument("--bam", metavar="bam_file", required=True, help="Sorted reads (BAM, fragment file or FragmentStore .npz)")
    p.add_argument("--bed", metavar="bed_file", help="Regions in which to get insertions")
    p.add_argument("--out", metavar="basename")
    p.add_argument("--cores", metavar="int", default=1, type=int, help="accepted for compatibility; the GPU replaces the pool")
    p.add_argument("--lower", metavar="int", default=0, type=int, help="lower limit on insert size")
    p.add_argument("--upper", metavar="int", default=2000, type=int, help="upper limit on insert size")


def add_ins_parser(sub):
    p = sub.add_parser("ins", help="pyatac function-- get insertions")
    _add_track_options(p)
    p.add_argument("--smooth", metavar="int", type=int, help="smoothing window for guassian smoothing.  default is no smoothing")
    p.add_argument("--not_atac", action="store_false", dest="atac", default=True, help="Don't use atac offsets")


def add_cov_parser(sub):
    p = sub.add_parser("cov", help="pyatac function-- get coverage")
    _add_track_options(p)
    p.add_argument("--window", metavar="int", type=int, default=121,
                   help="window for flat smoothing of coverage.  default is 121, should be odd")
    p.add_argument("--scale", metavar="float", type=float, default=10,
                   help="scaling value.  default is 10, corresponding to signal corresponding to # of fragment centers per 10 bp. "
                        "Use 1 for fragments per 1 bp.")
    p.add_argument("--not_atac", action="store_false", dest="atac", default=True, help="Don't use atac offsets")


def add_bias_parser(sub):
    p = sub.add_parser("bias", help="pyatac function-- compute Tn5 bias score")
    p.add_argument("--fasta", metavar="fasta_file", required=True, help="Accepts fasta file (or a FastaStore .npz)")
    p.add_argument("--pwm", metavar="Tn5_PWM", default="Human", help="PWM descriptor file or built-in name. Default is Human")
    p.add_argument("--bed", metavar="bed_file", help="Find only bias for these regions of the genome")
    p.add_argument("--out", metavar="output_basename", help="Basename for output")
    p.add_argument("--cores", metavar="int", default=1, type=int, help="accepted for compatibility; the GPU replaces the pool")


def add_counts_parser(sub):
    p = sub.add_parser("counts", help="pyatac function-- compute fragment counts within windows")
    p.add_argument("--bam", metavar="bam_file", required=True, help="Aligned reads (BAM, fragment file or FragmentStore .npz)")
    p.add_argument("--bed", metavar="bed_file", required=True, help="Windows in which to compute counts")
    p.add_argument("--out", metavar="output_basename", help="Basename for output")
    p.add_argument("--not_atac", action="store_false", dest="atac", default=True, help="Don't use atac offsets")
    p.add_argument("--lower", metavar="int", default=0, type=int, help="lower limit on insert size. Default is 0")
    p.add_argument("--upper", metavar="int", default=500, type=int, help="upper limit on insert size.  Default is 500")


def add_nucleotide_parser(sub):
    p = sub.add_parser("nucleotide", help="pyatac function-- get nucleotide (or di-nucleotide) content around sites")
    p.add_argument("--fasta", metavar="fasta_file", required=True, help="Accepts fasta file (or a FastaStore .npz)")
    p.add_argument("--bed", metavar="bed_file", required=True, help="Positions around which to get nucleotide frequencies")
    p.add_argument("--dinucleotide", action="store_true", default=False,
                   help="Compute dinucleotide frequencies instead of single nucleotide")
    p.add_argument("--up", metavar="int", default=250, type=int, help="Bases upstream of site to get frequencies for")
    p.add_argument("--down", metavar="int", default=250, type=int, help="Bases downstream of site to get frequencies for")
    p.add_argument("--strand", metavar="int", type=int, help="Column in bedfile with strand info (1-based)")
    p.add_argument("--out", metavar="output_basename", help="Basename for output")
    p.add_argument("--cores", metavar="int", default=1, type=int, help="accepted for compatibility; the GPU replaces the pool")
    p.add_argument("--norm", action="store_true", default=False, help="Normalize by background frequencies")


def add_signal_parser(sub):
    p = sub.add_parser("signal", help="pyatac function-- get signal around sites")
    p.add_argument("--bed", metavar="bed_file", required=True, help="Positions around which to get the signal")
    p.add_argument("--bg", metavar="bg_file", required=True, help="Accepts bedgraph file that is tabix indexed")
    p.add_argument("--sizes", metavar="genome_sizes_file", required=True, help="File with chromosome names in 1st col, sizes in 2nd")
    p.add_argument("--out", metavar="basename", help="basename for output")
    p.add_argument("--cores", metavar="int", type=int, default=1, help="accepted for compatibility; the GPU replaces the pool")
    p.add_argument("--all", action="store_true", default=False, help="output csv file (gzipped) with signal track around all sites")
    p.add_argument("--no_agg", action="store_true", default=False, help="Don't write the aggregate")
    p.add_argument("--up", metavar="int", type=int, default=250, help="bases upstream of site to look")
    p.add_argument("--down", metavar="int", type=int, default=250, help="bases downstream of site to look")
    p.add_argument("--weight", metavar="int", type=int, default=None, help="accepted for compatibility; ignored, like the reference")
    p.add_argument("--strand", metavar="int", type=int, default=None,
                   help="Column in which strand information is included if strand is to be used")
    p.add_argument("--exp", action="store_true", default=False, help="take exponent of value")
    p.add_argument("--positive", action="store_true", default=False, help="Only include positive signal")
    p.add_argument("--scale", action="store_true", default=False, help="scale each individual track by total signal value")
    p.add_argument("--norm", action="store_true", default=False, help="normalize aggregate track by number of intervals")


def add_split_parser(sub):
    p = sub.add_parser("split", help="split a single-cell fragment file by cell barcode into one store per cell group")
    p.add_argument("--fragments", metavar="fragment_file", required=True, help="Fragment file with the cell barcode in its fourth column")
    p.add_argument("--groups", metavar="table", required=True,
                   help="TAB-separated: barcode, group (without a second column every barcode listed is in the group 'selected')")
    p.add_argument("--header", action="store_true", default=False, help="The table's first line is a header")
    p.add_argument("--out", metavar="basename", help="Basename for output. Default is the fragment file's name without its suffixes")
    p.add_argument("--format", choices=("npz", "fragments"), default="npz",
                   help="Write every group as BASE.<group>.npz (default) or as BASE.<group>.tsv.gz with its .tbi")


def add_cells_parser(sub):
    p = sub.add_parser("cells", help="discover the cell barcodes of a single-cell fragment file, with per-cell QC counts")
    p.add_argument("--fragments", metavar="fragment_file", required=True, help="Fragment file with the cell barcode in its fourth column")
    p.add_argument("--min_fragments", metavar="int", default=1000, type=int, help="A cell passes with at least this many fragments. Default is 1000")
    p.add_argument("--max_nucleosome_signal", metavar="float", default=None, type=float,
                   help="A cell passes only if mono-nucleosomal / nucleosome-free fragments is at most this. Default is no such test")
    p.add_argument("--nfr_upper", metavar="int", default=147, type=int, help="Fragments shorter than this are nucleosome-free. Default is 147")
    p.add_argument("--mono_upper", metavar="int", default=294, type=int,
                   help="Fragments from --nfr_upper up to this (exclusive) are mono-nucleosomal. Default is 294")
    p.add_argument("--out", metavar="basename", help="Basename for output. Default is the fragment file's name without its suffixes")


def add_cellqc_parser(sub):
    p = sub.add_parser("cellqc", help="per-cell TSS enrichment and fraction of fragments in peaks of a single-cell fragment file")
    p.add_argument("--fragments", metavar="fragment_file", required=True, help="Fragment file with the cell barcode in its fourth column")
    p.add_argument("--cells", metavar="table", required=True,
                   help="TAB-separated table whose first column lists the barcodes, in order of first appearance (the table `split --groups` "
                        "takes and `cells` writes; a group column is not used).  Lines of a barcode the table does not list are left out")
    p.add_argument("--header", action="store_true", default=False, help="The table's first line is a header")
    p.add_argument("--tss", metavar="bed_file", help="Transcription start sites: every row is centred and counts as one site")
    p.add_argument("--strand", metavar="int", type=int, default=None, help="Column of --tss with strand information (1-based)")
    p.add_argument("--peaks", metavar="bed_file", help="Peaks: overlapping rows are merged, a fragment counts once")
    p.add_argument("--flank", metavar="int", default=1000, type=int, help="Bases on either side of a site that the profile covers. Default is 1000")
    p.add_argument("--center", metavar="int", default=500, type=int,
                   help="Insertions within this many bases of a site are the cell's signal. Default is 500")
    p.add_argument("--edge", metavar="int", default=100, type=int,
                   help="Insertions in the outermost this many bases of either flank are the cell's background. Default is 100")
    p.add_argument("--min_tss_enrichment", metavar="float", default=None, type=float,
                   help="A cell passes only with at least this TSS enrichment. Default is no such test")
    p.add_argument("--min_frip", metavar="float", default=None, type=float,
                   help="A cell passes only with at least this fraction of its fragments in peaks. Default is no such test")
    p.add_argument("--out", metavar="basename", help="Basename for output. Default is the fragment file's name without its suffixes")


def add_cellcounts_parser(sub):
    p = sub.add_parser("cellcounts", help="cell-by-window fragment count matrix of a single-cell fragment file")
    p.add_argument("--fragments", metavar="fragment_file", required=True, help="Fragment file with the cell barcode in its fourth column")
    p.add_argument("--bed", metavar="bed_file", required=True, help="Windows in which to compute counts: the rows of the matrix")
    p.add_argument("--cells", metavar="table", required=True,
                   help="TAB-separated table whose first column lists the barcodes: the columns of the matrix, in order of first appearance "
                        "(the table `split --groups` takes and `cells` writes; a group column is not used).  Barcodes are not discovered "
                        "from the fragment file here: lines of a barcode the table does not list are left out")
    p.add_argument("--header", action="store_true", default=False, help="The table's first line is a header")
    p.add_argument("--lower", metavar="int", default=0, type=int, help="lower limit on insert size. Default is 0")
    p.add_argument("--upper", metavar="int", default=500, type=int, help="upper limit on insert size.  Default is 500")
    p.add_argument("--out", metavar="basename", help="Basename for output. Default is the bed file's name without its last extension")
    p.add_argument("--format", choices=("mtx", "npz"), default="mtx",
                   help="BASE.cellcounts.mtx.gz with .barcodes.tsv and .regions.bed (default) or BASE.cellcounts.npz (CSR arrays)")


def add_cluster_parser(sub):
    p = sub.add_parser("cluster", help="cluster the cells of a cell-by-window count matrix: TF-IDF, LSI and k-means")
    p.add_argument("--counts", metavar="matrix", required=True,
                   help="BASE.cellcounts.npz or BASE.cellcounts.mtx.gz (with its .barcodes.tsv beside it) as `cellcounts` writes them")
    p.add_argument("--clusters", metavar="int", required=True, type=int, help="Number of clusters")
    p.add_argument("--components", metavar="int", default=30, type=int, help="LSI components kept for the embedding. Default is 30")
    p.add_argument("--oversample", metavar="int", default=10, type=int,
                   help="Further columns of the iterated block; components + oversample is at most 64. Default is 10")
    p.add_argument("--iterations", metavar="int", default=4, type=int, help="Rounds of subspace iteration. Default is 4")
    p.add_argument("--method", choices=("log", "linear"), default="log", help="log1p(10000 x TF-IDF) (default) or TF-IDF itself")
    p.add_argument("--binarize", action="store_true", default=False, help="Every count becomes 1")
    p.add_argument("--min_cells", metavar="int", default=1, type=int, help="Windows seen in fewer cells are dropped. Default is 1")
    p.add_argument("--max_depth_cor", metavar="float", default=0.75, type=float,
                   help="A component whose correlation with log10 of the cells' totals exceeds this in magnitude is removed. Default is 0.75")
    p.add_argument("--max_iter", metavar="int", default=100, type=int, help="Most k-means steps. Default is 100")
    p.add_argument("--seed", metavar="int", default=1, type=int, help="Seed of the block the iteration starts from. Default is 1")
    p.add_argument("--out", metavar="basename", help="Basename for output. Default is the matrix file's name without .cellcounts and its suffix")


def add_doublets_parser(sub):
    p = sub.add_parser("doublets", help="doublet score per cell: simulated doublets among the nearest neighbours in LSI space")
    p.add_argument("--counts", metavar="matrix", required=True,
                   help="BASE.cellcounts.npz or BASE.cellcounts.mtx.gz (with its .barcodes.tsv beside it) as `cellcounts` writes them")
    p.add_argument("--components", metavar="int", default=30, type=int, help="LSI components kept for the embedding. Default is 30")
    p.add_argument("--oversample", metavar="int", default=10, type=int,
                   help="Further columns of the iterated block; components + oversample is at most 64. Default is 10")
    p.add_argument("--iterations", metavar="int", default=4, type=int, help="Rounds of subspace iteration. Default is 4")
    p.add_argument("--method", choices=("log", "linear"), default="log", help="log1p(10000 x TF-IDF) (default) or TF-IDF itself")
    p.add_argument("--binarize", action="store_true", default=False, help="Every count becomes 1; a simulated doublet is the union")
    p.add_argument("--min_cells", metavar="int", default=1, type=int, help="Windows seen in fewer cells are dropped. Default is 1")
    p.add_argument("--max_depth_cor", metavar="float", default=0.75, type=float,
                   help="A component whose correlation with log10 of the cells' totals exceeds this in magnitude is removed. Default is 0.75")
    p.add_argument("--seed", metavar="int", default=1, type=int,
                   help="Seed of the block the iteration starts from and of the simulated pairs. Default is 1")
    p.add_argument("--ratio", metavar="float", default=2.0, type=float, help="Simulated doublets per kept cell, in (0, 8]. Default is 2.0")
    p.add_argument("--neighbors", metavar="int", default=None, type=int,
                   help="Neighbours k before the simulated ones are allowed for, in [1, 1024]. Default is round(0.5 sqrt(cells))")
    p.add_argument("--expected_rate", metavar="float", default=0.06, type=float, help="Expected doublet rate, in (0, 0.5]. Default is 0.06")
    p.add_argument("--filter_ratio", metavar="float", default=None, type=float,
                   help="Flag the int(F * cells^2 / 100000) highest-scoring cells, F in [0, 100]. Default is 1.0; excludes --max_score")
    p.add_argument("--max_score", metavar="float", default=None, type=float, help="Flag the cells that score above this; excludes --filter_ratio")
    p.add_argument("--out", metavar="basename", help="Basename for output. Default is the matrix file's name without .cellcounts and its suffix")


def add_coaccess_parser(sub):
    p = sub.add_parser("coaccess", help="the pairs of nearby windows that open and close together, by a correlation over the cells")
    p.add_argument("--counts", metavar="matrix", required=True,
                   help="BASE.cellcounts.npz or BASE.cellcounts.mtx.gz (with its .barcodes.tsv and .regions.bed) as `cellcounts` writes them")
    p.add_argument("--aggregate", metavar="table", help="TAB-separated: barcode, group (the table `cluster` writes). The counts are summed "
                   "per group first and the groups are the cells (metacells)")
    p.add_argument("--header", action="store_true", default=False, help="The table's first line is a header")
    p.add_argument("--binarize", action="store_true", default=False, help="Every entry of the matrix counts as 1 (before --aggregate)")
    p.add_argument("--min_cells", metavar="int", default=10, type=int,
                   help="A window is tested when at least this many cells have a count in it. Default is 10")
    p.add_argument("--max_distance", metavar="int", default=250000, type=int,
                   help="Two windows are paired when their centres are at most this far apart. Default is 250000")
    p.add_argument("--min_cor", metavar="float", default=0.5, type=float, help="A link has a correlation of at least this. Default is 0.5")
    p.add_argument("--fdr", metavar="float", default=0.05, type=float, help="A link has a q-value of at most this. Default is 0.05")
    p.add_argument("--out", metavar="basename", help="Basename for output. Default is the count matrix's name without .cellcounts and its suffix")


def add_genescores_parser(sub):
    p = sub.add_parser("genescores", help="gene activity per cell: insertions around every gene weighted by distance to the gene body")
    p.add_argument("--fragments", metavar="fragment_file", required=True, help="Fragment file with the cell barcode in its fourth column")
    p.add_argument("--cells", metavar="table", required=True,
                   help="TAB-separated table whose first column lists the barcodes: the columns of the matrix, in order of first appearance "
                        "(the table `cellcounts --cells` takes)")
    p.add_argument("--header", action="store_true", default=False, help="The table's first line is a header")
    p.add_argument("--genes", metavar="bed_file", required=True,
                   help="TAB-separated BED of genes: chrom, start, end, a name and a strand: the rows of the matrix, in file order")
    p.add_argument("--name", metavar="int", default=4, type=int, help="Column of the gene name, 1-based. Default is 4")
    p.add_argument("--strand", metavar="int", default=6, type=int, help="Column of the strand (`-` is minus, anything else plus). Default is 6")
    p.add_argument("--upstream", metavar="int", default=5000, type=int,
                   help="The gene body is extended this far upstream of the gene's start. Default is 5000")
    p.add_argument("--min_extend", metavar="int", default=1000, type=int,
                   help="The window reaches at least this far beyond the extended body. Default is 1000")
    p.add_argument("--max_extend", metavar="int", default=100000, type=int,
                   help="The window reaches at most this far beyond the extended body. Default is 100000")
    p.add_argument("--decay", metavar="int", default=5000, type=int, help="Distance over which the weight falls by e. Default is 5000")
    p.add_argument("--no_boundaries", action="store_true", default=False, help="Neighbouring genes do not stop a gene's window")
    p.add_argument("--unit", metavar="int", default=256, type=int,
                   help="The integer a weight of 1 is written as, 4 to 65536; lower it if a sum could pass 2^31. Default is 256")
    p.add_argument("--lower", metavar="int", default=0, type=int, help="lower limit on insert size. Default is 0")
    p.add_argument("--upper", metavar="int", default=1000, type=int, help="upper limit on insert size. Default is 1000")
    p.add_argument("--format", choices=("npz", "mtx"), default="npz",
                   help="BASE.genescores.npz (default; carries the gene names) or BASE.genescores.mtx.gz with .barcodes.tsv and .regions.bed")
    p.add_argument("--out", metavar="basename", help="Basename for output. Default is the gene file's name without its last extension")


def add_peaks_parser(sub):
    p = sub.add_parser("peaks", help="call enriched regions (peaks) from the insertions of a fragment store")
    p.add_argument("--bam", metavar="bam_file", required=True, help="Aligned reads (BAM, fragment file or FragmentStore .npz)")
    p.add_argument("--fasta", metavar="fasta_file", help="Chromosome lengths from this FASTA (or FastaStore .npz)")
    p.add_argument("--sizes", metavar="genome_sizes_file", help="Chromosome lengths from this file (names in 1st col, sizes in 2nd). "
                                                                "Without --fasta and --sizes the lengths are those of the reads' source")
    p.add_argument("--out", metavar="basename", help="Basename for output")
    p.add_argument("--half_width", metavar="int", default=75, type=int, help="Half-width of the pileup window. Default is 75")
    p.add_argument("--small", metavar="int", default=500, type=int, help="Half-width of the small local window. Default is 500")
    p.add_argument("--large", metavar="int", default=5000, type=int, help="Half-width of the large local window. Default is 5000")
    p.add_argument("--mlog10p", metavar="float", default=5.0, type=float,
                   help="A base is significant when its pileup has a Poisson tail probability of at most 10^-this. Default is 5")
    p.add_argument("--max_gap", metavar="int", default=75, type=int,
                   help="Significant bases with at most this many others between them are one region. Default is 75")
    p.add_argument("--min_length", metavar="int", default=150, type=int, help="Regions shorter than this are dropped. Default is 150")
    p.add_argument("--fixed_width", metavar="int", default=None, type=int,
                   help="Also write disjoint windows of this width around the summits, the most significant first")


def add_motifs_parser(sub):
    p = sub.add_parser("motifs", help="scan a genome, or the windows of a BED file, for the sites of TF motifs")
    p.add_argument("--fasta", metavar="fasta_file", required=True, help="Accepts fasta file (or a FastaStore .npz)")
    p.add_argument("--motifs", metavar="motif_file", required=True, help="Motifs in MEME minimal text format or JASPAR format")
    p.add_argument("--bed", metavar="bed_file", help="Windows to scan and to count matches in. Default is every chromosome whole")
    p.add_argument("--only", metavar="ID", nargs="+", help="Keep only the motifs with these ids")
    p.add_argument("--pvalue", metavar="float", default=1e-4, type=float,
                   help="A window is a hit when a score as high has at most this probability under the background. Default is 1e-4")
    p.add_argument("--pseudocount", metavar="float", default=0.8, type=float, help="Pseudocount of every motif column. Default is 0.8")
    p.add_argument("--bg", metavar="bg", nargs="+", default=["uniform"],
                   help="Background: uniform (default), regions (the base content of the scanned intervals) or four numbers a c g t")
    p.add_argument("--format", choices=("mtx", "npz"), default="mtx", help="Format of the window-by-motif matrix. Default is mtx")
    p.add_argument("--no_sites", action="store_true", default=False, help="Don't write the sites file")
    p.add_argument("--out", metavar="basename", help="Basename for output")


def add_deviations_parser(sub):
    p = sub.add_parser("deviations", help="per-cell motif accessibility deviations and z-scores from the count and the motif matrix")
    p.add_argument("--counts", metavar="matrix", required=True,
                   help="BASE.cellcounts.npz or BASE.cellcounts.mtx.gz (with its .barcodes.tsv and .regions.bed) as `cellcounts` writes them")
    p.add_argument("--motifs", metavar="matrix", required=True,
                   help="BASE.motifs.npz or BASE.motifs.mtx.gz (with its .names.tsv and .regions.bed) as `motifs --bed` writes them, "
                        "over the same BED")
    p.add_argument("--fasta", metavar="fasta_file", required=True, help="Accepts fasta file (or a FastaStore .npz): the windows' GC content")
    p.add_argument("--groups", metavar="table", help="TAB-separated: barcode, group (the table `cluster` writes): also write the mean z per group")
    p.add_argument("--header", action="store_true", default=False, help="The table's first line is a header")
    p.add_argument("--iterations", metavar="int", default=50, type=int, help="Background window sets, 2 to 1024. Default is 50")
    p.add_argument("--gc_bins", metavar="int", default=25, type=int, help="GC content bins of the background grid. Default is 25")
    p.add_argument("--acc_bins", metavar="int", default=25, type=int, help="Accessibility bins of the background grid. Default is 25")
    p.add_argument("--min_bin", metavar="int", default=10, type=int,
                   help="The grid is reduced until a bin holds at least this many windows on average. Default is 10")
    p.add_argument("--seed", metavar="int", default=1, type=int, help="Seed of the background draws. Default is 1")
    p.add_argument("--out", metavar="basename", help="Basename for output. Default is the count matrix's name without .cellcounts and its suffix")


def add_markers_parser(sub):
    p = sub.add_parser("markers", help="the windows that distinguish every cell group from the rest, by a rank-sum test")
    p.add_argument("--counts", metavar="matrix", required=True,
                   help="BASE.cellcounts.npz or BASE.cellcounts.mtx.gz (with its .barcodes.tsv and .regions.bed) as `cellcounts` writes them")
    p.add_argument("--groups", metavar="table", required=True, help="TAB-separated: barcode, group (the table `cluster` writes)")
    p.add_argument("--header", action="store_true", default=False, help="The table's first line is a header")
    p.add_argument("--min_cells", metavar="int", default=10, type=int,
                   help="A window is tested when at least this many kept cells have a count in it. Default is 10")
    p.add_argument("--fdr", metavar="float", default=0.05, type=float, help="A marker has a q-value of at most this. Default is 0.05")
    p.add_argument("--min_log2fc", metavar="float", default=0.5, type=float,
                   help="A marker has a pseudo-bulk log2 fold change of at least this. Default is 0.5")
    p.add_argument("--top", metavar="int", default=None, type=int, help="Cut every group's BED file at this many markers")
    p.add_argument("--out", metavar="basename", help="Basename for output. Default is the count matrix's name without .cellcounts and its suffix")


def pyatac_parser():
    from .. import __version__
    parser = argparse.ArgumentParser(prog="pyatac", description="pyatac: the Tn5 PWM, the fragment-size distribution, the per-base "
                                                                "insertion, coverage and Tn5 bias tracks, fragment counts per window, "
                                                                "nucleotide content and track signal around sites; a single-cell fragment file "
                                                                "split by cell group, its cell-by-window count matrix, the discovery "
                                                                "of its cells and their TSS enrichment and fraction of fragments in peaks; "
                                                                "enriched regions (peaks) of a fragment store; the sites of TF motifs in a genome; "
                                                                "per-cell motif accessibility deviations; marker windows of cell groups")
    parser.add_argument("--version", action="version", version="%(prog)s " + __version__)
    sub = parser.add_subparsers(dest="call")
    sub.required = True
    add_pwm_parser(sub)
    add_sizes_parser(sub)
    add_ins_parser(sub)
    add_cov_parser(sub)
    add_bias_parser(sub)
    add_counts_parser(sub)
    add_nucleotide_parser(sub)
    add_signal_parser(sub)
    add_cells_parser(sub)
    add_cellqc_parser(sub)
    add_split_parser(sub)
    add_cellcounts_parser(sub)
    add_doublets_parser(sub)
    add_cluster_parser(sub)
    add_deviations_parser(sub)
    add_markers_parser(sub)
    add_coaccess_parser(sub)
    add_genescores_parser(sub)
    add_peaks_parser(sub)
    add_motifs_parser(sub)
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
    elif args.call in ("ins", "cov"):
        from .trackfiles import MissingChromosomeError
        print("---------Getting insertions to make track---------------------------------------")
        try:
            if args.call == "ins":
                from .get_ins import get_ins
                get_ins(args)
            else:
                from .get_cov import get_cov
                get_cov(args)
        except (MissingChromosomeError, ValueError) as e:
            sys.stderr.write("pyatac %s: %s\n" % (args.call, e))
            return 1
    elif args.call == "bias":
        from .make_bias_track import BiasTrackError, make_bias_track
        print("---------Making Tn5 Bias Track---------------------------------------")
        try:
            make_bias_track(args)
        except BiasTrackError as e:
            sys.stderr.write("pyatac bias: %s\n" % e)
            return 1
    elif args.call == "counts":
        from .chunk import BedColumnError
        from .get_counts import CountsError, get_counts
        print("---------Getting fragment counts in windows---------------------------------------")
        try:
            get_counts(args)
        except (CountsError, BedColumnError) as e:
            sys.stderr.write("pyatac counts: %s\n" % e)
            return 1
    elif args.call == "nucleotide":
        from .chunk import BedColumnError
        from .get_nucleotide import NucleotideError, get_nucleotide
        print("---------Getting nucleotide content around sites---------------------------------------")
        try:
            get_nucleotide(args)
        except (NucleotideError, BedColumnError) as e:
            sys.stderr.write("pyatac nucleotide: %s\n" % e)
            return 1
    elif args.call == "signal":
        from .chunk import BedColumnError
        from .signal_around_sites import SignalError, get_signal
        print("---------Getting signal around sites---------------------------------------")
        print("plots are not produced: only the .agg.track.txt and .tracks.txt.gz files are written")
        try:
            get_signal(args)
        except (SignalError, BedColumnError) as e:
            sys.stderr.write("pyatac signal: %s\n" % e)
            return 1
    elif args.call == "cells":
        from .._lib import NatacError
        from .get_cells import CellsError, get_cells
        print("---------Discovering cells---------------------------------------")
        try:
            get_cells(args)
        except (CellsError, NatacError) as e:
            sys.stderr.write("pyatac cells: %s\n" % e)
            return 1
    elif args.call == "cellqc":
        from .._lib import NatacError
        from .cellgroups import CellGroupError
        from .chunk import BedColumnError
        from .get_cellqc import CellQCError, get_cellqc
        print("---------Getting per-cell TSS enrichment and FRiP---------------------------------------")
        print("plots are not produced: only the .cellqc files are written")
        try:
            get_cellqc(args)
        except (CellQCError, BedColumnError, CellGroupError, NatacError) as e:
            sys.stderr.write("pyatac cellqc: %s\n" % e)
            return 1
    elif args.call == "split":
        from .._lib import NatacError
        from .cellgroups import CellGroupError, split_cells
        print("---------Splitting fragments by cell group---------------------------------------")
        try:
            split_cells(args)
        except (CellGroupError, NatacError) as e:
            sys.stderr.write("pyatac split: %s\n" % e)
            return 1
    elif args.call == "cellcounts":
        from .._lib import NatacError
        from .cellgroups import CellGroupError
        from .chunk import BedColumnError
        from .get_cellcounts import get_cellcounts
        from .get_counts import CountsError
        print("---------Getting the cell-by-window count matrix---------------------------------------")
        try:
            get_cellcounts(args)
        except (CountsError, BedColumnError, CellGroupError, NatacError) as e:
            sys.stderr.write("pyatac cellcounts: %s\n" % e)
            return 1
    elif args.call == "doublets":
        from .._lib import NatacError
        from .get_cluster import ClusterError
        from .get_doublets import get_doublets
        print("---------Scoring the cells of the count matrix for doublets----------------------------")
        try:
            get_doublets(args)
        except (ClusterError, NatacError) as e:
            sys.stderr.write("pyatac doublets: %s\n" % e)
            return 1
    elif args.call == "cluster":
        from .._lib import NatacError
        from .get_cluster import ClusterError, get_cluster
        print("---------Clustering the cells of the count matrix---------------------------------------")
        try:
            get_cluster(args)
        except (ClusterError, NatacError) as e:
            sys.stderr.write("pyatac cluster: %s\n" % e)
            return 1
    elif args.call == "deviations":
        from .._lib import NatacError
        from .cellgroups import CellGroupError
        from .get_deviations import DeviationsError, get_deviations
        print("---------Getting motif deviations per cell---------------------------------------")
        try:
            get_deviations(args)
        except (DeviationsError, CellGroupError, NatacError) as e:
            sys.stderr.write("pyatac deviations: %s\n" % e)
            return 1
    elif args.call == "markers":
        from .._lib import NatacError
        from .cellgroups import CellGroupError
        from .get_markers import MarkersError, get_markers
        print("---------Getting marker windows per cell group-----------------------------------")
        try:
            get_markers(args)
        except (MarkersError, CellGroupError, NatacError) as e:
            sys.stderr.write("pyatac markers: %s\n" % e)
            return 1
    elif args.call == "coaccess":
        from .._lib import NatacError
        from .cellgroups import CellGroupError
        from .get_coaccess import CoaccessError, get_coaccess
        print("---------Getting co-accessible window pairs----------------------------------------")
        try:
            get_coaccess(args)
        except (CoaccessError, CellGroupError, NatacError) as e:
            sys.stderr.write("pyatac coaccess: %s\n" % e)
            return 1
    elif args.call == "genescores":
        from .._lib import NatacError
        from .cellgroups import CellGroupError
        from .get_genescores import GenescoresError, get_genescores
        print("---------Getting gene activity scores per cell-------------------------------------")
        try:
            get_genescores(args)
        except (GenescoresError, CellGroupError, NatacError) as e:
            sys.stderr.write("pyatac genescores: %s\n" % e)
            return 1
    elif args.call == "peaks":
        from .._lib import NatacError
        from .get_peaks import PeaksError, get_peaks
        print("---------Calling enriched regions---------------------------------------")
        try:
            get_peaks(args)
        except (PeaksError, NatacError) as e:
            sys.stderr.write("pyatac peaks: %s\n" % e)
            return 1
    elif args.call == "motifs":
        from .._lib import NatacError
        from .chunk import BedColumnError
        from .get_motifs import MotifsError, get_motifs
        print("---------Scanning for motif sites---------------------------------------")
        try:
            get_motifs(args)
        except (MotifsError, BedColumnError, NatacError) as e:
            sys.stderr.write("pyatac motifs: %s\n" % e)
            return 1
    return 0


def main(argv=None):
    return pyatac_main(pyatac_parser().parse_args(argv))


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
