"""Corpus for the boundary tests: small non-bottommost jobs whose level-below
and grandparent files have boundary user keys next to, shorter than and
longer than the job's own keys.

Compaction::KeyNotExistsBeyondOutputLevel decides whether a tombstone is
dropped, CompactionOutputs::UpdateGrandparentBoundaryInfo where output files
are cut; both compare job keys with file boundaries in raw bytewise order
(bytes, then length).  Every job here comes with

  * `expected`: the survivor list in plain Python, `bytes` comparison only,
    where the job is simple enough to state exactly (MODEL jobs: no
    snapshots, one record per user key; a Put survives, a Delete survives
    iff some level-below file has smallest <= key <= largest);
  * `legacy_kw()`: the same job with every boundary replaced by what a
    compare of zero-padded 16-byte words sees of it (`legacy_bound`), and
    `legacy_expected` for general-key MODEL jobs, where that compare also
    cuts the job key; tests/test_bounds_cpu.py requires the jobs of the
    groups in SEPARATING to give another result under it, so that each of
    them can tell the two semantics apart, and the rest to give the same.

Built once per process and shared by the CPU and GPU tests; nothing here
touches the GPU.  Inputs are written with oracle.build_sst.
"""
import functools
import os
import random

import oracle

TYPE_DELETION, TYPE_VALUE, TYPE_SINGLE_DELETION = 0, 1, 7
FILE_SIZE = 1000  # level-below file sizes are not looked at
MIB = 1 << 20

# groups whose jobs must give another result under the padded compare, and
# groups whose jobs must give the same
SEPARATING = ("long", "short", "u8", "general", "gp", "mix")
NON_SEPARATING = ("same", "oneside", "gp_same")
# "oneside": a boundary that is longer than the job keys as a file's LARGEST,
# or shorter as its SMALLEST.  Padding moves such a boundary only across
# strings that are no job key (largest K+"x" -> K: a U-byte key u with
# K < u <= K+"x" does not exist; smallest K0-minus-zeros -> K0 likewise), so
# no input can separate the two semantics there.  The jobs stay: a fix that
# breaks ties on length the wrong way round fails them.


def k16(i):
    return b"k%015d" % i


def k8(i):
    return b"u%07d" % i


def legacy_bound(b, ulen):
    """The boundary that raw order must be given to reproduce a compare of
    zero-padded 16-byte words against `ulen`-byte job keys (ulen <= 16):
    bytes past 16 are cut, and a shorter boundary, or one that is longer
    only by zero bytes, is the ulen-byte key it pads to.  For ulen == 16 this
    is b[:16] right-padded with zeros.  ulen 0 = general-key mode: b[:16]."""
    b = b[:16]
    if ulen == 0:
        return b
    while len(b) > ulen and b.endswith(b"\0"):
        b = b[:-1]
    return b.ljust(ulen, b"\0")


def pad16(b):
    return b[:16].ljust(16, b"\0")


class Job:
    """kvs_runs: [[(ukey, seq, type, value)]], each run sorted in internal
    key order.  levels: [[(smallest, largest)]] below the output level."""

    def __init__(self, name, group, kvs_runs, levels=(), grandparents=(),
                 model=True, ulen=16, **job_kw):
        self.name = name
        self.group = group
        self.kvs_runs = kvs_runs
        self.levels = [list(lv) for lv in levels]
        self.grandparents = list(grandparents)
        self.model = model
        self.ulen = ulen  # uniform user-key length, 0 = general-key mode
        self.job_kw = dict(compression=0, bottommost_level=0)
        self.job_kw.update(job_kw)
        assert sum(len(r) for r in kvs_runs) <= 8200

    # ---- inputs
    @functools.cached_property
    def ssts(self):
        return [oracle.build_sst([(oracle.make_ikey(k, s, t), v)
                                  for k, s, t, v in kvs])
                for kvs in self.kvs_runs]

    def write_inputs(self, directory):
        """-> the job's `runs` argument (one file per run)."""
        paths = []
        for i, sst in enumerate(self.ssts):
            p = os.path.join(str(directory), "%s_in%d.sst" % (self.name, i))
            if not os.path.exists(p):
                with open(p, "wb") as f:
                    f.write(sst)
            paths.append([p])
        return paths

    # ---- job descriptors
    def _kw(self, f):
        kw = dict(self.job_kw)
        if self.levels or "levels_below_valid" in kw:
            kw["levels_below"] = [[(f(sm), f(lg), FILE_SIZE) for sm, lg in lv]
                                  for lv in self.levels]
        if self.grandparents:
            kw["grandparents"] = [(f(sm), f(lg), sz)
                                  for sm, lg, sz in self.grandparents]
        return kw

    def kw(self):
        return self._kw(lambda b: b)

    def legacy_kw(self):
        return self._kw(lambda b: legacy_bound(b, self.ulen))

    # ---- the plain-Python model
    @property
    def tombstones(self):
        return [k for kvs in self.kvs_runs for k, s, t, v in kvs
                if t != TYPE_VALUE]

    def _survivors(self, covered):
        assert self.model
        kw = self.job_kw
        out = []
        for k, s, t, v in sorted(e for kvs in self.kvs_runs for e in kvs):
            if t == TYPE_VALUE:
                # bottommost + no snapshot: the sequence number is zeroed
                out.append((oracle.make_ikey(
                    k, 0 if kw["bottommost_level"] else s, t), v))
            elif kw["bottommost_level"]:
                continue
            elif not kw.get("levels_below_valid", 1) or covered(k):
                out.append((oracle.make_ikey(k, s, t), v))
        return out

    @property
    def expected(self):
        return self._survivors(lambda k: any(
            sm <= k <= lg for lv in self.levels for sm, lg in lv))

    @property
    def legacy_expected(self):
        """Survivors if job key and boundary are both compared as zero-padded
        16-byte words only (exact for every mode, MODEL jobs only)."""
        return self._survivors(lambda k: any(
            pad16(sm) <= pad16(k) <= pad16(lg)
            for lv in self.levels for sm, lg in lv))


# ------------------------------------------------------------ level below
def one_record_runs(keys, rng, put_every=7, protect=()):
    """One record per user key over two runs: a Delete, or a Put for every
    `put_every`-th key that is not in `protect` (the keys a case is about
    stay tombstones)."""
    protect = set(protect)
    runs = [[], []]
    for i, k in enumerate(sorted(keys)):
        put = i % put_every == put_every // 2 and k not in protect
        runs[rng.randrange(2)].append(
            (k, 100 + i, TYPE_VALUE if put else TYPE_DELETION,
             b"value-%d" % i if put else b""))
    return runs


def _lb(name, group, keys, levels, seed, ulen=16, put_every=7, **kw):
    near = {b for lv in levels for f in lv for b in f}
    ks = sorted(keys)
    protect = set()
    for b in near:  # every job key within two places of a boundary
        at = sum(1 for k in ks if k < b)
        protect.update(ks[max(0, at - 2):at + 3])
    return Job(name, group, one_record_runs(keys, random.Random(seed),
                                            put_every, protect),
               levels, ulen=ulen, **kw)


def _same_jobs():
    even = [k16(i) for i in range(0, 120, 2)]
    jobs = [
        # key == smallest and key == largest (and their neighbours)
        _lb("same_on_bounds", "same", even, [[(k16(20), k16(30))]], 1),
        # boundaries that are no job key: the key just below smallest and
        # the key just above largest are the nearest ones
        _lb("same_beside_bounds", "same", even, [[(k16(21), k16(31))]], 2),
        # before the first file, in the gap, after the last file
        _lb("same_gaps", "same", even,
            [[(k16(10), k16(14)), (k16(20), k16(24))]], 3),
        _lb("same_point_file", "same", even,
            [[(k16(20), k16(20)), (k16(31), k16(31)), (k16(40), k16(40))]], 4),
        _lb("same_touching", "same", even,
            [[(k16(10), k16(20)), (k16(20), k16(30))]], 5),
        _lb("same_three_levels", "same", even,
            [[(k16(0), k16(8))], [(k16(40), k16(48))], [(k16(20), k16(28))]],
            6),
        _lb("same_empty_level", "same", even,
            [[(k16(0), k16(8))], [], [(k16(20), k16(28))]], 7),
    ]
    # files per level: the binary search at lo == e and at both ends
    for n in (1, 2, 3, 7, 8, 33):
        keys = [k16(i) for i in range(10 * n + 10)]
        files = [(k16(10 * f + 2), k16(10 * f + 6)) for f in range(n)]
        jobs.append(_lb("same_files_%d" % n, "same", keys, [files], 10 + n,
                        put_every=3))
    return jobs


def _long_jobs():
    """U=16 inputs, boundaries K + "x"*j of 17..24 bytes, K a job key."""
    keys = [k16(i) for i in range(100)]
    sm = [(k16(10 * j) + b"x" * j, k16(10 * j + 5)) for j in range(1, 9)]
    lg = [(k16(10 * j - 5), k16(10 * j) + b"x" * j) for j in range(1, 9)]
    both = [(k16(10 * j) + b"x" * j, k16(10 * j + 5) + b"x" * (9 - j))
            for j in range(1, 9)]
    return [_lb("long_smallest", "long", keys, [sm], 21),
            _lb("long_largest", "oneside", keys, [lg], 22),
            _lb("long_both", "long", keys, [both], 23)]


def z16(i, j):
    """16-byte key number i whose last j bytes are zero."""
    return (b"s%012d" % i + b"aaa")[:16 - j] + b"\0" * j


def _short_jobs():
    """U=16 inputs, some keys end in 1..3 zero bytes; boundaries are such a
    key without its zero bytes (15, 14 and 13 bytes)."""
    keys = [z16(i, j) for i in range(40) for j in range(4)]
    lg = [(z16(10 * j - 3, 0), z16(10 * j, j)[:16 - j]) for j in (1, 2, 3)]
    sm = [(z16(10 * j, j)[:16 - j], z16(10 * j + 3, 0)) for j in (1, 2, 3)]
    return [_lb("short_largest", "short", keys, [lg], 31),
            _lb("short_smallest", "oneside", keys, [sm], 32)]


def _u8_jobs():
    """U=8 inputs, boundaries K + "\\0"*j, j = 1..8."""
    keys = [k8(i) for i in range(100)]
    sm = [(k8(10 * j) + b"\0" * j, k8(10 * j + 5)) for j in range(1, 9)]
    lg = [(k8(10 * j - 5), k8(10 * j) + b"\0" * j) for j in range(1, 9)]
    return [_lb("u8_smallest", "u8", keys, [sm], 41, ulen=8),
            _lb("u8_largest", "oneside", keys, [lg], 42, ulen=8)]


P16 = b"p" * 16


def g24(i):
    return P16 + b"%08d" % i


def g48(i):
    return P16 + b"%08d" % i + b"q" * 24


def general_keys():
    """24- and 48-byte keys alternating, all sharing their first 16 bytes."""
    return [g24(i) if i % 2 == 0 else g48(i) for i in range(80)]


GENERAL_FILES = [
    (g24(10), g48(21)),                  # bounds that are job keys
    (g48(41)[:47], g24(50) + b"\0"),     # bounds between job keys
]


def _general_jobs():
    fam = ([b"aa", b"ab", b"ab\0", b"ab\0\0", b"abc", b"abc\0", b"abd",
            b"b" * 20] +
           [b"ac%d" % i * n for i in range(6) for n in (1, 5, 12)])
    jobs = [_lb("general_24_48", "general", general_keys(), [GENERAL_FILES],
                51, ulen=0)]
    # b"ab" < b"ab\0" < b"abc": a point file on each member keeps only it
    for tag, member in (("ab", b"ab"), ("ab0", b"ab\0"), ("abc", b"abc")):
        jobs.append(_lb("general_family_" + tag, "general", fam,
                        [[(member, member)]], 52, ulen=0))
    # a 60-byte boundary, longer than any accepted key: 48-byte job keys
    # that are its prefix lie below it
    keys = [g48(i) for i in range(40)]
    jobs.append(_lb("general_bound_60", "general", keys,
                    [[(g48(10) + b"z" * 12, g48(20) + b"z" * 12)]], 53,
                    ulen=0))
    return jobs


def _switch_jobs():
    keys = [k16(i) for i in range(0, 120, 2)]
    files = [[(k16(20), k16(30))]]
    return [_lb("switch_levels_below_invalid", "switch", keys, files, 61,
                levels_below_valid=0),
            _lb("switch_bottommost", "switch", keys, files, 62,
                bottommost_level=1)]


def mixed_record_runs(keys, rng):
    """Delete, SingleDelete and Put, 1 to 4 versions per key over 3 runs.  A
    key is written either with Put/SingleDelete (a SingleDelete only right
    after one Put) or with Put/Delete, never both (the reference's
    SingleDelete contract).  -> (runs, highest sequence number)"""
    seq = 1
    runs = [[], [], []]
    for k in sorted(keys):
        sd_key = rng.random() < 0.4
        last_put = False
        for _ in range(rng.randint(1, 4)):
            if sd_key and last_put and rng.random() < 0.6:
                e, last_put = (k, seq, TYPE_SINGLE_DELETION, b""), False
            elif sd_key or rng.random() < 0.5:
                e, last_put = (k, seq, TYPE_VALUE, b"v%d" % seq), True
            else:
                e, last_put = (k, seq, TYPE_DELETION, b""), False
            runs[rng.randrange(3)].append(e)
            seq += 1
    for r in runs:
        r.sort(key=lambda e: (e[0], -((e[1] << 8) | e[2])))
    return runs, seq - 1


def _mix_jobs():
    """Checked against the oracle only."""
    long_files = [(k16(10 * j) + b"x" * j, k16(10 * j + 5) + b"x" * (9 - j))
                  for j in range(1, 9)]
    jobs = []
    for layout, keys, files, ulen, seed in (
            ("long", [k16(i) for i in range(100)], long_files, 16, 71),
            ("general", general_keys(), GENERAL_FILES, 0, 72)):
        for snap in (0, 1):
            runs, top = mixed_record_runs(keys, random.Random(seed))
            kw = {}
            if snap:
                kw = dict(snapshots=[top // 2],
                          earliest_write_conflict_snapshot=top // 2)
            jobs.append(Job("mix_%s_%s" % (layout, "snap" if snap else "nosnap"),
                            "mix", runs, [files], model=False, ulen=ulen, **kw))
    return jobs


@functools.lru_cache(maxsize=None)
def level_below_jobs():
    return tuple(_same_jobs() + _long_jobs() + _short_jobs() + _u8_jobs() +
                 _general_jobs() + _switch_jobs() + _mix_jobs())


# ------------------------------------------------------------ grandparents
# 8000 Puts with 100-byte values give about 0.9 MiB of output; with
# target_file_size = 1 MiB nothing is cut on size alone, so every cut comes
# from a grandparent rule of ShouldStopBefore (compaction_outputs.cc:231-352):
#   "cut": max_compaction_bytes of a few MiB, files every GP_STEP keys: the
#          overlapped-bytes rule cuts where a key crosses a boundary;
#   "dyn": max_compaction_bytes = 1 TiB and one or two late files: only the
#          dynamic-file-size rule is left, which cuts at a crossing once the
#          output file holds 50 % + 5 % per crossing of the target size
#          (about 117 bytes per entry: 55 % at entry 4950, 65 % at 5850).
GP_ENTRIES = 8000
GP_STEP, GP_SPAN = 300, 200
GP_UNBOUNDED = 1 << 40


def _gp_value(i):
    return (b"%010d" % i) * 10  # 100 bytes


def gz16(i):
    return b"k%012d" % i + b"\0\0\0"


def gz8(i):
    return b"u%05d" % i + b"\0\0"


def _strip(k):
    return k.rstrip(b"\0")


def _gp_job(name, group, key, gps, ulen, max_compaction_bytes):
    """GP_ENTRIES Puts key(i) in two runs against the grandparent files
    `gps` = [(smallest, largest, file size)]."""
    kvs = [(key(i), 1 + i, TYPE_VALUE, _gp_value(i))
           for i in range(GP_ENTRIES)]
    assert all(a[1] <= b[0] and a[0] <= a[1] for a, b in zip(gps, gps[1:]))
    return Job(name, group, [kvs[0::2], kvs[1::2]], grandparents=gps,
               ulen=ulen, target_file_size=MIB,
               max_compaction_bytes=max_compaction_bytes)


def _gp_jobs():
    jobs = []
    steps = range(0, GP_ENTRIES - GP_SPAN, GP_STEP)
    for u, key, zkey, ext in ((16, k16, gz16, b"x"), (8, k8, gz8, b"\0")):
        def long_file(g, j):
            # 17..24 (U=8: 9..16) bytes, the first U a survivor key
            return (key(g) + ext * j, key(g + GP_SPAN) + ext * j, MIB)

        def tie_files(largest_of_first):
            # a single file, then two adjacent files whose common boundary
            # is a survivor key T: with a budget of 2.5 MiB the third MiB is
            # entered at T, so an output file starts there, and what it
            # counts as overlapped includes the file before T iff that
            # file's largest == T (compaction_outputs.cc:218-227)
            out = []
            for g in steps:
                t = zkey(g + 150)
                out += [(zkey(g), zkey(g + 50), MIB),
                        (zkey(g + 100), largest_of_first(t), MIB),
                        (t, zkey(g + GP_SPAN), MIB)]
            return out

        def tie_late(largest_of_first):
            t = zkey(6400)
            return [(zkey(4000), largest_of_first(t), MIB),
                    (t, zkey(7500), MIB)]

        layouts = (
            ("long_cut", "gp", key, 3 * MIB,
             [long_file(g, 1 + i % 8) for i, g in enumerate(steps)]),
            # the file is entered, and the output cut, at 55 %
            ("long_dyn", "gp", key, GP_UNBOUNDED, [long_file(5200, 4)]),
            # boundaries that are a survivor key without its trailing zero
            # bytes.  Only the largest tells the semantics apart, where the
            # key leaves the file: the file size lets the budget run out
            # between entering (100 keys into the output file) and leaving
            ("short_cut", "gp", zkey, 3 * MIB,
             [(_strip(zkey(g)), _strip(zkey(g + GP_SPAN)), 3 * MIB - 16384)
              for g in steps]),
            # entered below 55 %, left above 60 %
            ("short_dyn", "gp", zkey, GP_UNBOUNDED,
             [(_strip(zkey(4000)), _strip(zkey(6000)), MIB)]),
            # largest_j == smallest_j+1 == a survivor key: equal bytes ...
            ("tie_equal_cut", "gp_same", zkey, 5 * MIB // 2,
             tie_files(lambda t: t)),
            # ... and equal only after padding
            ("tie_nul_cut", "gp", zkey, 5 * MIB // 2, tie_files(_strip)),
            # without a budget the tie changes nothing that a rule looks at
            # (both semantics leave one file and enter the next at T)
            ("tie_equal_dyn", "gp_same", zkey, GP_UNBOUNDED,
             tie_late(lambda t: t)),
            ("tie_nul_dyn", "gp_same", zkey, GP_UNBOUNDED, tie_late(_strip)),
        )
        for shape, group, kf, mcb, gps in layouts:
            jobs.append(_gp_job("gp%d_%s" % (u, shape), group, kf, gps, u,
                                mcb))
    return jobs


@functools.lru_cache(maxsize=None)
def grandparent_jobs():
    return tuple(_gp_jobs())


def all_jobs():
    return level_below_jobs() + grandparent_jobs()


def by_name(name):
    return {j.name: j for j in all_jobs()}[name]


def names(jobs):
    return [j.name for j in jobs]
