"""Per-haplotype coverage tracks from lcr_hap_coverage's segments (include/lcr.h): bedGraph text per class and the
dense planes.  Class 0 is the unassigned reads, 1 / 2 the haplotypes as the HP tag names them."""
import numpy as np

TRACKS = ((1, "h1"), (2, "h2"), (0, "unassigned"))   # class, file suffix: PREFIX.<suffix>.bedgraph


def track_runs(segments, k):
    """the runs of class k's track: [(start, end, value)] -- segments whose value in that class is 0 are skipped, abutting segments with an
    equal value are merged (the triple's run-length encoding splits finer than one class does).  segments: one contig's, ordered by start."""
    start = np.asarray(segments["start0"], np.int64)
    end = start + np.asarray(segments["len"], np.int64)
    val = np.asarray(segments["n"], np.int64).reshape(-1, 3)[:, k]
    keep = val != 0
    start, end, val = start[keep], end[keep], val[keep]
    if start.size == 0:
        return []
    first = np.ones(start.size, bool)
    first[1:] = (start[1:] != end[:-1]) | (val[1:] != val[:-1])
    i0 = np.flatnonzero(first)
    i1 = np.append(i0[1:], start.size) - 1
    return list(zip(start[i0].tolist(), end[i1].tolist(), val[i0].tolist()))


def format_bedgraph(contig, segments, k):
    """bedGraph lines `contig\\tstart\\tend\\tvalue` (0-based half-open, no track header line) of class k"""
    return "".join("%s\t%d\t%d\t%d\n" % (contig, s, e, v) for s, e, v in track_runs(segments, k))


def expand(segments, start0, length):
    """the dense 3 x length depth planes (uint32) of the window [start0, start0 + length) from the segments that lie inside it"""
    d = np.zeros((3, int(length)), np.uint32)
    for s, n, v in zip(np.asarray(segments["start0"], np.int64).tolist(), np.asarray(segments["len"], np.int64).tolist(),
                       np.asarray(segments["n"], np.uint32).reshape(-1, 3)):
        lo = s - int(start0)
        if lo < 0 or lo + n > length:
            raise ValueError("segment [%d, %d) outside the window [%d, %d)" % (s, s + n, start0, start0 + length))
        d[:, lo:lo + n] = v[:, None]
    return d


class TrackWriter:
    """Writes PREFIX.h1.bedgraph, PREFIX.h2.bedgraph and PREFIX.unassigned.bedgraph contig by contig, in the order given.  Checks that
    the lines of a file are sorted and non-overlapping inside a contig (a chunk-order bug raises ValueError) and sums the covered bases."""

    def __init__(self, prefix):
        self.paths = {k: "%s.%s.bedgraph" % (prefix, name) for k, name in TRACKS}
        self.files = {k: open(p, "w") for k, p in self.paths.items()}
        self.bases = [0, 0, 0]
        self.segments = 0

    def add_contig(self, contig, segments):
        """segments: the contig's records in chunk order (their region field is not read)"""
        self.segments += len(segments)
        for k, f in self.files.items():
            last = -1
            for s, e, v in track_runs(segments, k):
                if s < last or e <= s:
                    raise ValueError("hap coverage: %s [%d, %d) of track %d is not behind the line that ends at %d" % (contig, s, e, k, last))
                last = e
                self.bases[k] += (e - s) * v
                f.write("%s\t%d\t%d\t%d\n" % (contig, s, e, v))

    def close(self):
        for f in self.files.values():
            f.close()
