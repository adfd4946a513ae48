"""linkage_qc: the allele every alignment carries at a set of variable sites,
and how those alleles co-occur across alignments.

A pileup is a sum over reads: it cannot tell five positions with independent
5 % errors from ONE 5 % sub-population that carries all five (a second clone
in the prep).  This module keeps the per-read alleles at up to 128 sites and
counts every site pair's joint alleles (include/mpc_linkage.h has the
definition; DESIGN.md "linkage_qc").

  run           alleles u8[N][K] + pair u32[K][K][8][8] of a batch of records:
                K_lnkparse + K_lnkplanes + K_lnkpair in ONE mpc_linkage_run on the
                GPU (libmpc.so), or the scalar host walk (device="cpu")
  pairs         the pair counts of a given allele matrix
  select_sites  candidate sites from coverage.run rows
  pair_stats    r^2 and the `linked` call of one site pair, from exact integers
  qc            per PAF: one coverage.run, one site selection, one run; verdict

The defaults (minor fraction 0.05, minor count 10, r^2 0.1, joint count 10)
are starting values nobody has validated on real runs.
"""
import numpy as np

from . import _native, coverage, engine

MAX_SITES = 128  # mpc_linkage.h MPC_LNK_MAX_SITES
CODES = 8
MIN_MINOR_FRACTION, MIN_MINOR_COUNT, MIN_R2, MIN_JOINT, MAX_HAPLOTYPES = 0.05, 10, 0.1, 10, 50
_LETTER = ".ACGTN"  # codes 1-6


class LinkageError(ValueError):
    """Input that cannot be measured (the CLI exits 1)."""


def base_key(p):
    return 2 * p + 1


def gap_key(p):
    return 2 * p


def site_label(key):
    """'<1-based position>:base|gap' of a site key (gap: before that base)."""
    return "{}:{}".format(key // 2 + 1, "base" if key & 1 else "gap")


host_lib = coverage.host_lib


def tile_bytes():
    """cs bytes K_lnkparse takes per tile (no GPU needed)."""
    return engine.lib().mpc_linkage_tile_bytes()


def scratch_bytes(n_records, n_sites):
    return engine.lib().mpc_linkage_scratch_bytes(n_records, n_sites)


def run(cs, cs_off, tstart, rec_sample, lengths, site_off, site_key, device=0, threads=0):
    """(alleles u8[N][K], pair u32[K][K][8][8]) of the records (cs bytes,
    cs_off[n + 1], tstart[n], rec_sample[n]) over samples of the given lengths
    at the sites site_off[S + 1] / site_key[K] (2p + 1: base p, 2p: the gap before
    base p).  Raises LinkageError naming the smallest malformed or out-of-range
    record, or what is wrong with the tables."""
    site_off = np.ascontiguousarray(site_off, np.int64)
    site_key = np.ascontiguousarray(site_key, np.int64)
    n, S, K = len(tstart), len(lengths), len(site_key)
    more = [(len(site_off) != S + 1, "site_off needs one entry per target and one more"),
            (not 1 <= K <= MAX_SITES, "{} sites: outside [1, {}]".format(K, MAX_SITES))]
    cs, cs_off, tstart, rec_sample, pos_off = coverage.batch_front(LinkageError, cs, cs_off, tstart, rec_sample, lengths, more)
    if device == "cpu":
        L = host_lib()
        alleles = np.zeros((n, K), np.uint8)
        pair = np.zeros((K, K, CODES, CODES), np.uint32)
        status = np.zeros(2, np.int32)
        _native.host_check(L, "linkage", LinkageError, L.mpc_linkage_host(
            cs.ctypes.data, cs_off.ctypes.data, tstart.ctypes.data, rec_sample.ctypes.data, n, pos_off.ctypes.data, S,
            site_off.ctypes.data, site_key.ctypes.data, K, alleles.ctypes.data, pair.ctypes.data, status.ctypes.data, threads))
    else:
        with _native.Device(device, "host walk") as d:
            torch, dev = d.torch, d.dev
            # the int64 tables first, then rec_sample, then the cs bytes
            at, d_blob = d.put_all([cs_off, tstart, pos_off, site_off, site_key, rec_sample, cs])
            d_alleles = torch.empty((n, K), dtype=torch.uint8, device=dev)
            d_pair = torch.empty((K, K, CODES, CODES), dtype=torch.int32, device=dev)
            d_scratch = torch.empty(max(8, scratch_bytes(n, K) // 8), dtype=torch.int64, device=dev)
            d_status = torch.empty(2, dtype=torch.int32, device=dev)
            d.check(d.lib.mpc_linkage_run(at[6], at[0], at[1], at[5], n, at[2], S, at[3], at[4], K, d_alleles.data_ptr(),
                                          d_pair.data_ptr(), d_scratch.data_ptr(), d_status.data_ptr(), d.stream),
                    refused=LinkageError)
            status = d_status.cpu().numpy()
            alleles = d_alleles.cpu().numpy()
            pair = d_pair.cpu().numpy().view(np.uint32)
    coverage.raise_status(LinkageError, status)
    return alleles, pair


def pairs(alleles, device=0, threads=0):
    """pair u32[K][K][8][8] of an allele matrix u8[N][K] (codes are taken & 7):
    K_lnkplanes + K_lnkpair, or the host count (device="cpu")."""
    alleles = np.ascontiguousarray(alleles, np.uint8)
    if alleles.ndim != 2:
        raise LinkageError("alleles must be a matrix [records][sites]")
    n, K = alleles.shape
    if not 1 <= K <= MAX_SITES:
        raise LinkageError("{} sites: outside [1, {}]".format(K, MAX_SITES))
    if device == "cpu":
        L = host_lib()
        pair = np.zeros((K, K, CODES, CODES), np.uint32)
        _native.host_check(L, "linkage", LinkageError,
                           L.mpc_linkage_pairs_host(alleles.ctypes.data, n, K, pair.ctypes.data, threads))
        return pair
    with _native.Device(device, "host walk") as d:
        torch, dev = d.torch, d.dev
        d_alleles = torch.empty((max(n, 1), K), dtype=torch.uint8, device=dev)
        if n:
            d_alleles[:n].copy_(torch.from_numpy(alleles))
        d_pair = torch.empty((K, K, CODES, CODES), dtype=torch.int32, device=dev)
        d_scratch = torch.empty(max(8, scratch_bytes(n, K) // 8), dtype=torch.int64, device=dev)
        d.check(d.lib.mpc_linkage_pairs(d_alleles.data_ptr(), n, K, d_pair.data_ptr(), d_scratch.data_ptr(), d.stream),
                refused=LinkageError)
        return d_pair.cpu().numpy().view(np.uint32)


def site_fractions(rows, pos_off, regions):
    """[(fraction, sample, key, minor count)] of every candidate site of every
    sample's region [lo, hi): base p for lo <= p < hi with m = mismatch +
    deleted over depth + deleted; the gap before base p for lo <= p < hi, and
    the gap at L when hi = L, with m = insertion[p] over depth + deleted at p
    (at p = L: of L - 1).  Sites nothing covers are left out."""
    out = []
    for s, (lo, hi) in enumerate(regions):
        blk = np.asarray(rows[int(pos_off[s]):int(pos_off[s + 1])], np.int64)
        L = len(blk) - 1
        if L < 1:
            continue
        cover = blk[:L, 0] + blk[:L, 1]
        minor = blk[:L, 2] + blk[:L, 1]
        for p in range(lo, hi):
            if cover[p] > 0:
                out.append((int(minor[p]) / int(cover[p]), s, base_key(p), int(minor[p])))
        for p in range(lo, hi + 1 if hi == L else hi):
            den = int(cover[min(p, L - 1)])
            if den > 0:
                out.append((int(blk[p, 3]) / den, s, gap_key(p), int(blk[p, 3])))
    return out


def select_sites(rows, pos_off, regions, min_minor_fraction=MIN_MINOR_FRACTION, min_minor_count=MIN_MINOR_COUNT,
                 max_sites=MAX_SITES):
    """(site_off int64[S + 1], site_key int64[K], dropped): the sites of
    site_fractions with minor count >= min_minor_count and fraction >=
    min_minor_fraction.  More than max_sites: the highest fractions are kept
    (ties: the smaller sample, then the smaller key) and `dropped` counts the rest."""
    cand = [c for c in site_fractions(rows, pos_off, regions) if c[3] >= min_minor_count and c[0] >= min_minor_fraction]
    cand.sort(key=lambda c: (-c[0], c[1], c[2]))
    keep = sorted((s, key) for _, s, key, _ in cand[:max_sites])
    site_off = np.zeros(len(regions) + 1, np.int64)
    for s, _ in keep:
        site_off[s + 1] += 1
    return np.cumsum(site_off), np.array([k for _, k in keep], np.int64), max(0, len(cand) - max_sites)


def major_code(pair, i):
    """The most frequent code >= 1 at site i (ties: the smallest code)."""
    diag = [int(pair[i, i, a, a]) for a in range(CODES)]
    return max(range(1, CODES), key=lambda a: (diag[a], -a))


def pair_stats(pair, i, j, min_r2=MIN_R2, min_joint=MIN_JOINT):
    """dict(major_i, major_j, n, x, y, n11, r2, linked) of the site pair: over
    the n records with both codes >= 1, x and y the minor counts at i and j,
    n11 the count minor at both; r2 = (n n11 - x y)^2 / (x (n - x) y (n - y))
    from Python integers with one division, 0.0 when that denominator is 0."""
    mi, mj = major_code(pair, i), major_code(pair, j)
    cell = [[int(pair[i, j, a, b]) for b in range(CODES)] for a in range(CODES)]
    n = sum(cell[a][b] for a in range(1, CODES) for b in range(1, CODES))
    x = sum(cell[a][b] for a in range(1, CODES) for b in range(1, CODES) if a != mi)
    y = sum(cell[a][b] for a in range(1, CODES) for b in range(1, CODES) if b != mj)
    n11 = sum(cell[a][b] for a in range(1, CODES) for b in range(1, CODES) if a != mi and b != mj)
    den = x * (n - x) * y * (n - y)
    r2 = (n * n11 - x * y) ** 2 / den if den else 0.0
    return dict(major_i=mi, major_j=mj, n=n, x=x, y=y, n11=n11, r2=r2,
                linked=n11 >= min_joint and n * n11 > x * y and r2 >= min_r2)


def haplotypes(alleles, keys):
    """[(string, count)] of the records covered at every site (keys: their site
    keys), by descending count, then by string: '.' reference, ACGTN the
    substituted base, '-' a deleted base, '+' an insertion at a gap site."""
    sub = alleles[(alleles >= 1).all(axis=1)] if len(keys) else alleles[:0]
    if not len(sub):
        return []
    uniq, counts = np.unique(sub, axis=0, return_counts=True)
    text = ["".join(("-" if k & 1 else "+") if c == 7 else _LETTER[c - 1] for c, k in zip(row.tolist(), keys)) for row in uniq]
    return sorted(zip(text, counts.tolist()), key=lambda t: (-t[1], t[0]))


def read_sites(path):
    """{target: sorted site keys} of a --sites file: lines
    'target<TAB>1-based position<TAB>base|gap' (gap: before that base)."""
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line or line.startswith("#"):
                continue
            col = line.split("\t")
            if len(col) != 3 or not col[1].isdigit() or int(col[1]) < 1 or col[2] not in ("base", "gap"):
                raise LinkageError("{}: line {}: expected target<TAB>1-based position<TAB>base|gap".format(path, no))
            p = int(col[1]) - 1
            out.setdefault(col[0], set()).add(base_key(p) if col[2] == "base" else gap_key(p))
    return {t: sorted(k) for t, k in out.items()}


def qc(paf_paths, sites=None, min_minor_fraction=MIN_MINOR_FRACTION, min_minor_count=MIN_MINOR_COUNT, expected=None,
       region=None, all_alignments=False, min_r2=MIN_R2, min_joint=MIN_JOINT, device=0, threads=0):
    """dict(blocks, verdict): one block per (paf, target).  Per PAF: one
    coverage.run, one site selection (or `sites` = {target: keys}) and one
    linkage run.  verdict: "PASS" iff no site pair of any target is linked."""
    core = coverage.expected_core(expected, LinkageError)
    blocks, linked_any, named = [], False, set()
    for path in paf_paths:
        try:
            d = coverage.read_paf(path, 1 if all_alignments else 0, threads)
        except coverage.CoverageError as e:
            raise LinkageError(str(e))
        lengths, names = d["lengths"], d["names"]
        if not lengths:
            raise LinkageError("no alignment in {}".format(path))
        regions = coverage.target_regions(path, names, lengths, core, region, LinkageError)
        batch = (d["cs"], d["cs_off"], d["tstart"], d["target"], lengths)
        try:
            if sites is None:
                cov = coverage.run(*batch, regions, 0, device, threads, tend=d["tend"])
                site_off, site_key, dropped = select_sites(cov["rows"], cov["pos_off"], regions, min_minor_fraction,
                                                           min_minor_count)
            else:
                per = [sites.get(name, []) for name in names]
                named.update(n for n in names if n in sites)
                site_off = np.cumsum([0] + [len(k) for k in per]).astype(np.int64)
                site_key = np.array([k for ks in per for k in ks], np.int64)
                dropped = 0
                if len(site_key) > MAX_SITES:
                    raise LinkageError("{}: {} sites named, at most {} fit one run".format(path, len(site_key), MAX_SITES))
            alleles = pair = None
            if len(site_key):
                alleles, pair = run(*batch, site_off, site_key, device, threads)
        except (LinkageError, coverage.CoverageError) as e:
            raise LinkageError("{} (records in the order of the kept PAF lines of {})".format(e, path))
        for s, name in enumerate(names):
            a, b = int(site_off[s]), int(site_off[s + 1])
            keys = [int(k) for k in site_key[a:b]]
            stats = [(i - a, j - a, pair_stats(pair, i, j, min_r2, min_joint)) for i in range(a, b) for j in range(i + 1, b)]
            sel = d["target"] == s
            blk = dict(paf=str(path), target=name, length=lengths[s], records=int(sel.sum()), region=regions[s], keys=keys,
                       dropped=dropped, pairs=stats,
                       counts=[[int(pair[i, i, c, c]) for c in range(CODES)] for i in range(a, b)],
                       majors=[major_code(pair, i) for i in range(a, b)],
                       haplotypes=haplotypes(alleles[sel][:, a:b], keys) if keys else [])
            linked_any = linked_any or any(st["linked"] for _, _, st in stats)
            blocks.append(blk)
    if sites is not None and set(sites) - named:
        raise LinkageError("no PAF has the target(s) {} of the sites file".format(", ".join(sorted(set(sites) - named))))
    return dict(blocks=blocks, verdict="FAIL" if linked_any else "PASS")
