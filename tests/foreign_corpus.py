"""Input corpus for the foreign-input tests: SSTs whose data blocks were NOT
written by the project's own codec or with its default table geometry.

Built once per process and shared (CPU coverage tests assert the op-form
conditions on exactly the blocks the GPU tests decode).  Everything is
seeded; nothing here touches the GPU.
"""
import functools
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import foreign_snappy as fs  # noqa: E402
import oracle  # noqa: E402

DEC_MAX = 4992  # dcw_k_decode.h: LDS decoders take n <= DEC_MAX, usize <= DEC_MAX
SNAPPY = 1
TYPE_DELETION, TYPE_VALUE = 0, 1


def ukey(i):
    return b"k%014d" % i  # 15 bytes, uniform: the worker's fast key path


class Recorder:
    """data_block_codec that applies a per-block policy and keeps every
    (policy name, raw block, stored type, payload) it produced."""

    def __init__(self, choose, seed=0):
        self.choose = choose  # (block index, raw) -> policy name/"raw"/"dcw"
        self.seed = seed
        self.blocks = []

    def __call__(self, raw):
        idx = len(self.blocks)
        name = self.choose(idx, raw)
        if callable(name):  # a ready-made payload builder (malformed streams)
            payload = name(raw)
            self.blocks.append(("custom", raw, SNAPPY, payload))
            return SNAPPY, payload
        if name == "raw":
            self.blocks.append((name, raw, 0, raw))
            return None
        if name == "dcw":
            payload = oracle.snappy_compress(raw)
        else:
            payload = fs.POLICIES[name](raw, seed=self.seed * 7919 + idx)
        self.blocks.append((name, raw, SNAPPY, payload))
        return SNAPPY, payload


def branch_of(ctype, n, usize):
    """Which k_decompress branch a stored block takes, from its sizes."""
    if ctype == 0:
        return "raw"
    return "lds" if n <= DEC_MAX and usize <= DEC_MAX else "fallback"


def survivors(runs_kvs):
    """Plain-Python expectation for a bottommost compaction without
    snapshots: newest version of each user key wins, deletions vanish with
    what they cover, survivors have their sequence number zeroed."""
    newest = {}
    for kvs in runs_kvs:
        for uk, seq, typ, val in kvs:
            if uk not in newest or seq > newest[uk][0]:
                newest[uk] = (seq, typ, val)
    return [(oracle.make_ikey(uk, 0, TYPE_VALUE), val)
            for uk, (seq, typ, val) in sorted(newest.items())
            if typ == TYPE_VALUE]


def build_run(kvs, choose, seed=0, **table_opts):
    """kvs: [(ukey, seq, type, value)] sorted by ukey (one version per key
    per run).  -> (sst bytes, Recorder)."""
    rec = Recorder(choose, seed)
    entries = [(oracle.make_ikey(k, s, t), v) for k, s, t, v in kvs]
    sst = oracle.build_sst(entries, oracle.default_table_opts(**table_opts),
                           data_block_codec=rec)
    return sst, rec


class Job:
    def __init__(self, name, runs, **job_kw):
        self.name = name
        self.runs = runs  # [(kvs, sst bytes, Recorder)]
        self.job_kw = job_kw  # extra make_job fields (none so far)

    @property
    def ssts(self):
        return [r[1] for r in self.runs]

    @property
    def expected(self):
        return survivors([r[0] for r in self.runs])

    def blocks(self):
        for _, _, rec in self.runs:
            yield from rec.blocks

    def write_inputs(self, directory):
        """-> the job's `runs` argument (one file per run)."""
        paths = []
        for i, sst in enumerate(self.ssts):
            p = os.path.join(str(directory), "%s_in%d.sst" % (self.name, i))
            with open(p, "wb") as f:
                f.write(sst)
            paths.append([p])
        return paths


# ------------------------------------------------------------ value shapes
def mixed_values(n, rng, far=()):
    """Block-like content: random values (long literals), byte runs and
    short periods (overlapping copies), repeats of earlier values (long,
    chunked matches).  `far`: extra look-back distances, in values, for the
    repeats (long back-references in large blocks)."""
    vals = []
    for i in range(n):
        r = rng.random()
        if r < 0.40 or i < 4:
            v = rng.randbytes(rng.randint(20, 120))
        elif r < 0.55:
            v = bytes([rng.randrange(256)]) * rng.randint(10, 200)
        elif r < 0.75:
            back = rng.choice((1, 2, 3) + tuple(far))
            v = vals[max(0, i - back)]
            if rng.random() < 0.5:
                v = v[:len(v) // 2] + b"\xa5" + v[len(v) // 2:]
        else:
            period = rng.randint(2, 12)
            pat = rng.randbytes(period)
            v = (pat * 100)[:rng.randint(20, 150)]
        vals.append(v)
    return vals


def two_runs(n0, n1, rng, far=()):
    """Run 0: keys 0,2,4..; run 1 (newer): keys 0,3,6.., a quarter of them
    deletions — half shadow or delete a run-0 key, half are new."""
    v0 = mixed_values(n0, rng, far)
    v1 = mixed_values(n1, rng, far)
    kv0 = [(ukey(2 * i), 1 + i, TYPE_VALUE, v0[i]) for i in range(n0)]
    kv1 = []
    for i in range(n1):
        dele = rng.random() < 0.25
        kv1.append((ukey(3 * i), 100000 + i,
                    TYPE_DELETION if dele else TYPE_VALUE,
                    b"" if dele else v1[i]))
    return kv0, kv1


# ------------------------------------------------------------- corpus (a)
@functools.lru_cache(maxsize=None)
def policy_job(policy):
    rng = random.Random(0xF0 + sorted(fs.POLICIES).index(policy))
    kv0, kv1 = two_runs(900, 700, rng)
    runs = []
    for r, kvs in enumerate((kv0, kv1)):
        sst, rec = build_run(kvs, lambda i, raw: policy, seed=r + 1)
        runs.append((kvs, sst, rec))
    return Job("pol_" + policy, runs)


@functools.lru_cache(maxsize=None)
def directed_job():
    """Every offset x length of the directed sweep, one value each, spread
    over two runs (greedy policy)."""
    rng = random.Random(0xD1)
    cases = [(o, ln) for o in fs.DIRECTED_OFFSETS
             for ln in fs.DIRECTED_LENGTHS]
    kvs = [[], []]
    for i, (o, ln) in enumerate(cases):
        kvs[i % 2].append((ukey(i), 1 + i, TYPE_VALUE,
                           fs.directed_value(o, ln, rng)))
    # overlap between the runs: run 1 re-writes and deletes a few run-0 keys
    for j, i in enumerate(range(0, len(cases), 20)):
        kvs[1].append((ukey(i), 10000 + i, TYPE_DELETION if j % 2 else
                       TYPE_VALUE, b"" if j % 2 else b"rewritten-%d" % i))
    runs = []
    for r in range(2):
        run = sorted(kvs[r])
        sst, rec = build_run(run, lambda i, raw: "greedy", seed=r + 11)
        runs.append((run, sst, rec))
    return Job("directed", runs), cases


@functools.lru_cache(maxsize=None)
def mixed_job():
    """One file whose blocks rotate raw / project codec / foreign policies."""
    rng = random.Random(0xA3)
    kv0, kv1 = two_runs(900, 700, rng)
    rota = ("raw", "dcw", "greedy", "dcw", "raw", "fragmented", "greedy_tag3",
            "all_literal")
    runs = []
    for r, kvs in enumerate((kv0, kv1)):
        sst, rec = build_run(kvs, lambda i, raw: rota[i % len(rota)],
                             seed=r + 21)
        runs.append((kvs, sst, rec))
    return Job("mixed", runs)


# ------------------------------------------------------------- corpus (b)
ENTRY_OVERHEAD = 1 + 1 + 2 + 23 + 8  # shared, non_shared, vlen(2B), ikey, restart array


def _compressible(n, rng):
    pat = rng.randbytes(37)
    return (pat * (n // 37 + 1))[:n]


def _random(n, rng):
    return rng.randbytes(n)


@functools.lru_cache(maxsize=None)
def decmax_job():
    """One entry per block (block_size 64: every entry flushes), values sized
    so the uncompressed block / the stream land on each side of DEC_MAX.
    -> (Job, [(label, policy, wanted usize)] for run 0's blocks)."""
    rng = random.Random(0xB2)
    plan = []  # (label, policy, usize, value maker)
    for us in (DEC_MAX - 1, DEC_MAX, DEC_MAX + 1, 6000):
        plan.append(("compressible_%d" % us, "greedy", us, _compressible))
    # all_literal: n = usize + 2 (preamble) + 3 (tag + 2 length bytes)
    for us in (DEC_MAX - 6, DEC_MAX - 5, DEC_MAX - 4, DEC_MAX - 1, DEC_MAX):
        plan.append(("all_literal_%d" % us, "all_literal", us, _random))
    plan.append(("fragmented_3500", "fragmented", 3500, _random))
    plan.append(("raw_4000", "raw", 4000, _random))
    plan.append(("raw_5003", "raw", 5003, _random))
    # a block whose greedy stream ends on a copy: the value ends with the
    # bytes of the block's own restart trailer (num_restarts = 1)
    tail = b"\x01\x00\x00\x00" + b"\x00" * 8
    plan.append(("ends_on_copy", "greedy", 300,
                 lambda n, rng: _random(n - len(tail), rng) + tail))
    kv0 = []
    for i, (_, _, us, make) in enumerate(plan):
        kv0.append((ukey(10 * i), 1 + i, TYPE_VALUE,
                    make(us - ENTRY_OVERHEAD, rng)))
    sst0, rec0 = build_run(kv0, lambda i, raw: plan[i][1], seed=31,
                           block_size=64)
    # run 1: default geometry, shadows one boundary block and deletes another
    v1 = mixed_values(60, rng)
    kv1 = [(ukey(10 * i + 5), 5000 + i, TYPE_VALUE, v1[i]) for i in range(60)]
    kv1.append((ukey(10), 9000, TYPE_DELETION, b""))
    kv1.append((ukey(40), 9001, TYPE_VALUE, b"shadow"))
    kv1.sort()
    sst1, rec1 = build_run(kv1, lambda i, raw: "greedy", seed=32)
    job = Job("decmax", [(kv0, sst0, rec0), (kv1, sst1, rec1)])
    return job, [(p[0], p[1], p[2]) for p in plan]


# ------------------------------------------------------------- corpus (c)
# (block_size, block_restart_interval, index_block_restart_interval, codec);
# the two runs of one job use different geometries.  Every value of every
# axis appears with both codecs.
GEOMETRY_JOBS = (
    ((512, 1, 1, "greedy"), (65536, 64, 4, "raw")),
    ((4096, 2, 4, "raw"), (16384, 16, 1, "greedy")),
    ((16384, 64, 4, "greedy"), (512, 16, 1, "raw")),
    ((65536, 1, 4, "greedy"), (4096, 64, 1, "greedy")),
    ((65536, 16, 1, "greedy"), (16384, 2, 4, "raw")),
    ((512, 2, 4, "greedy"), (4096, 1, 1, "raw")),
    ((4096, 16, 4, "greedy"), (512, 64, 4, "greedy")),
    ((16384, 1, 1, "raw"), (65536, 2, 1, "raw")),
)
_GEOM_ENTRIES = {512: 160, 4096: 700, 16384: 1100, 65536: 2300}


@functools.lru_cache(maxsize=None)
def geometry_job(idx):
    rng = random.Random(0xC0 + idx)
    geoms = GEOMETRY_JOBS[idx]
    n0, n1 = (_GEOM_ENTRIES[g[0]] for g in geoms)
    # repeats of values ~30 and ~350 entries back: offsets above 2048 and
    # above 32768 inside the 16 KiB / 64 KiB blocks
    kv0, kv1 = two_runs(n0, n1, rng, far=(30, 350))
    runs = []
    for r, (kvs, (bs, ri, iri, codec)) in enumerate(zip((kv0, kv1), geoms)):
        sst, rec = build_run(kvs, lambda i, raw, c=codec: c, seed=41 + r,
                             block_size=bs, block_restart_interval=ri,
                             index_block_restart_interval=iri)
        runs.append((kvs, sst, rec))
    return Job("geom%d" % idx, runs)


# ------------------------------------------------------------- corpus (e)
def _lit(data):
    out = bytearray()
    fs._emit_literal(out, data, 0, len(data))
    return bytes(out)


def malformed_streams(raw):
    """Fixed set of malformed streams for one raw block (>= 200 bytes).  Each
    is a case the decoders bounds-check before touching memory."""
    pre = fs.put_varint32(len(raw))
    head = pre + _lit(raw[:100])  # 100 valid bytes produced first
    return {
        "copy_offset_0": head + bytes([(7 << 2) | 2, 0, 0]) + _lit(raw[108:]),
        "copy_offset_gt_produced":
            head + bytes([(7 << 2) | 2, 101, 0]) + _lit(raw[108:]),
        "literal_past_input": head + bytes([60 << 2, 99]) + raw[100:150],
        "literal_past_ulen":
            fs.put_varint32(120) + _lit(raw[:100]) + _lit(raw[100:130]),
        "copy_past_ulen":
            fs.put_varint32(120) + _lit(raw[:100]) + bytes([(63 << 2) | 2, 50, 0]),
        "end_mid_copy1": head + bytes([(2 << 2) | 1]),
        "end_mid_copy2": head + bytes([(7 << 2) | 2, 50]),
        "end_mid_copy3": head + bytes([(7 << 2) | 3, 50, 0]),
        "end_mid_literal_ext1": head + bytes([60 << 2]),
        "end_mid_literal_ext2": head + bytes([61 << 2, 99]),
        "end_mid_literal_ext3": head + bytes([62 << 2, 99, 0]),
        "end_mid_literal_ext4": head + bytes([63 << 2, 99, 0, 0]),
        "short_of_ulen": pre + _lit(raw[:-1]),
        "varint_6_bytes": b"\x80\x80\x80\x80\x80\x01" + _lit(raw),
    }


MALFORMED_NAMES = tuple(malformed_streams(bytes(200)))
# one more at a size the global-memory fallback decodes (usize > DEC_MAX)
MALFORMED_FALLBACK = "fallback_copy_offset_gt_produced"


@functools.lru_cache(maxsize=None)
def malformed_input(name):
    """-> (sst bytes, the malformed stream): a small greedy-coded file whose
    second data block is the named malformed stream behind a valid trailer
    checksum."""
    rng = random.Random(0xE5)
    if name == MALFORMED_FALLBACK:
        vals = [_compressible(6000, rng) for _ in range(3)]
        opts = dict(block_size=64)

        def bad(raw):
            return (fs.put_varint32(len(raw)) + _lit(raw[:100]) +
                    bytes([(7 << 2) | 2, 101, 0]) + _lit(raw[108:]))
    else:
        vals = mixed_values(150, rng)
        opts = {}

        def bad(raw):
            return malformed_streams(raw)[name]
    kvs = [(ukey(i), 1 + i, TYPE_VALUE, v) for i, v in enumerate(vals)]
    sst, rec = build_run(kvs, lambda i, raw: bad if i == 1 else "greedy",
                         seed=51, **opts)
    assert len(rec.blocks) >= 3 and rec.blocks[1][0] == "custom"
    return sst, rec.blocks[1][3]


@functools.lru_cache(maxsize=None)
def good_small_job():
    """The job run after every refusal: small, foreign-coded, LDS path."""
    rng = random.Random(0xE6)
    kv0, kv1 = two_runs(120, 90, rng)
    runs = []
    for r, kvs in enumerate((kv0, kv1)):
        sst, rec = build_run(kvs, lambda i, raw: "greedy_tag3", seed=61 + r)
        runs.append((kvs, sst, rec))
    return Job("good_small", runs)


# -------------------------------------------------------------- the whole
def decoder_jobs():
    """Corpus (a) + (b): what every decoder variant runs."""
    return ([policy_job(p) for p in sorted(fs.POLICIES)] +
            [directed_job()[0], mixed_job(), decmax_job()[0]])


def all_jobs():
    return decoder_jobs() + [geometry_job(i)
                             for i in range(len(GEOMETRY_JOBS))]
