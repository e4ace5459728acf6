"""CPU side of the foreign-input harness: the plain-Python snappy helpers
against the oracle decoder, the oracle's data-block codec hook, the op-form
coverage of the corpus the GPU tests decode, and the host decoder fuzzers
under tools/dec_host_fuzz (which nothing else builds or runs)."""
import os
import random
import shutil
import subprocess
import sys
from collections import Counter

import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_corpus as fc  # noqa: E402
import foreign_snappy as fs  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sample_blocks():
    rng = random.Random(5)
    yield b""
    yield b"a"
    yield b"abc"
    yield b"abcd" * 3
    yield rng.randbytes(4000)  # incompressible: one literal, 2-byte length
    yield rng.randbytes(70000)  # 3-byte literal length
    yield b"\x00" * 5000
    far = rng.randbytes(300)
    yield far + rng.randbytes(66000) + far  # offset >= 65536: natural tag 3
    vals = fc.mixed_values(60, rng)
    yield b"".join(b"\x00\x17%c" % (len(v) & 0x7F) + fc.ukey(i) + v
                   for i, v in enumerate(vals))


@pytest.mark.parametrize("policy", sorted(fs.POLICIES))
def test_policies_round_trip(policy):
    for i, x in enumerate(_sample_blocks()):
        s = fs.POLICIES[policy](x, seed=i)
        assert fs.decode(s) == x
        assert oracle.snappy_uncompress(s) == x
        assert fs.parse(s)[0] == len(x)


def test_walk_classifies_forms():
    x = random.Random(6).randbytes(300)
    c = fs.walk(fs.all_literal(x))
    assert c == Counter(ops=1, lit_ext2=1)
    c = fs.walk(fs.all_literal(x[:61]))
    assert c == Counter(ops=1, lit_ext1=1)
    c = fs.walk(fs.greedy(x[:20] + b"z" * 40))
    assert c["lit_ext0"] >= 1 and c["overlap"] == 1 and c["off_1_7"] == 1
    far = x[:8] + bytes(70000) + x[:8]
    c = fs.walk(fs.greedy(far))
    assert c["copy_tag3"] == 1
    # the project codec's own streams walk too
    assert fs.walk(oracle.snappy_compress(x + x))["ops"] >= 2


def test_directed_values_give_exact_copies():
    rng = random.Random(7)
    for off in fs.DIRECTED_OFFSETS:
        for ln in fs.DIRECTED_LENGTHS:
            # as in a block: the key's last byte (top of the seq) is 0
            x = rng.randbytes(8) + b"\0" + fs.directed_value(off, ln, rng)
            s = fs.greedy(x)
            assert fs.decode(s) == x
            assert oracle.snappy_uncompress(s) == x
            ops = fs.parse(s)[1]
            copies = [o for o in ops if o.kind == "copy"]
            assert copies and all(o.offset == off for o in copies), (off, ln)
            assert sum(o.length for o in copies) == ln, (off, ln)
            for o in copies:  # tag 1 exactly where the format allows it
                want = 1 if 4 <= o.length <= 11 and off < 2048 else 2
                assert o.form == want, (off, ln)


def test_decode_rejects_malformed():
    raw = random.Random(8).randbytes(400)
    for name, s in fc.malformed_streams(raw).items():
        with pytest.raises(fs.SnappyError):
            fs.decode(s)
        with pytest.raises(fs.SnappyError):
            fs.parse(s)
        with pytest.raises(ValueError):
            oracle.snappy_uncompress(s)


# ---------------------------------------------------------- the codec hook
def _entries(n, seed):
    rng = random.Random(seed)
    return [(oracle.make_ikey(fc.ukey(i), 1 + i, 1),
             rng.randbytes(rng.randint(0, 90)) * rng.randint(1, 3))
            for i in range(n)]


def test_hook_absent_or_raw_changes_no_byte():
    es = _entries(400, 1)
    for comp in (0, 1):
        opts = oracle.default_table_opts(compression=comp)
        plain = oracle.build_sst(es, opts)
        assert oracle.build_sst(es, opts, data_block_codec=None) == plain
    # "store raw" from the hook == an uncompressed build
    opts = oracle.default_table_opts(compression=0)
    assert oracle.build_sst(es, opts, data_block_codec=lambda raw: None) == \
        oracle.build_sst(es, opts)
    # the project codec through the hook == the built-in snappy path for
    # blocks that pass its ratio check (these all do: values repeat)
    es2 = [(k, b"v" * 80) for k, _ in es]
    opts = oracle.default_table_opts(compression=1)
    a = oracle.build_sst(es2, opts)
    b = oracle.build_sst(
        es2, opts, data_block_codec=lambda raw: (1, oracle.snappy_compress(raw)))
    # index blocks are compressed by the builder in both; only data blocks differ
    assert a == b


def test_hook_sst_reads_back_and_skips_ratio_check():
    es = _entries(500, 2)
    seen = []

    def codec(raw):
        seen.append(raw)
        # fragmented expands incompressible blocks: stored regardless
        return 1, fs.fragmented(raw, seed=len(seen))

    sst = oracle.build_sst(es, data_block_codec=codec)
    assert oracle.read_sst(sst) == es
    assert len(seen) > 5
    assert len(sst) > len(oracle.build_sst(es))  # expansion was kept
    # data blocks only: every block the hook saw parses as a data block
    for raw in seen:
        assert int.from_bytes(raw[-4:], "little") >= 1


def test_hook_exception_propagates():
    def codec(raw):
        raise KeyError("boom")

    with pytest.raises(KeyError):
        oracle.build_sst(_entries(50, 3), data_block_codec=codec)


# ------------------------------------------------------ corpus properties
@pytest.fixture(scope="module")
def corpus_blocks():
    """(job name, policy, raw, type, payload) for every data block the GPU
    tests read."""
    out = []
    for job in fc.all_jobs():
        for name, raw, ctype, payload in job.blocks():
            out.append((job.name, name, raw, ctype, payload))
    return out


def test_corpus_streams_decode_everywhere(corpus_blocks):
    for job, name, raw, ctype, payload in corpus_blocks:
        if ctype == 0:
            assert payload == raw
            continue
        assert fs.decode(payload) == raw, (job, name)
        assert oracle.snappy_uncompress(payload) == raw, (job, name)


def test_corpus_ssts_read_back():
    for job in fc.all_jobs():
        for kvs, sst, _ in job.runs:
            want = [(oracle.make_ikey(k, s, t), v) for k, s, t, v in kvs]
            assert oracle.read_sst(sst) == want, job.name
        assert len(job.expected) > 0


def test_corpus_coverage_conditions(corpus_blocks):
    """Guards against the GPU tests quietly going soft: every decoder path
    the issue names must be present in the streams they decode."""
    total = Counter()
    overlap17 = set()  # offsets 1..16 with an overlapping copy of len >= 17
    max_chunks = 0
    max_ops = 0
    ends_1byte_literal = ends_copy = False
    max_offset = 0
    for job, name, raw, ctype, payload in corpus_blocks:
        if ctype == 0 or name == "dcw":
            continue
        ops = fs.parse(payload)[1]
        total += fs.walk(payload)
        max_ops = max(max_ops, len(ops))
        for o in ops:
            if o.kind == "copy":
                max_offset = max(max_offset, o.offset)
                if o.offset <= 16 and o.offset < o.length and o.length >= 17:
                    overlap17.add(o.offset)
        max_chunks = max([max_chunks] + fs.chunked_matches(ops))
        last = ops[-1]
        assert last.end == len(payload)
        ends_1byte_literal |= last.kind == "lit" and last.length == 1
        ends_copy |= last.kind == "copy"
    for form in ("lit_ext0", "lit_ext1", "lit_ext2"):
        assert total[form] > 0, form
    for form in ("copy_tag1", "copy_tag2", "copy_tag3"):
        assert total[form] > 0, form
    for bucket in ("off_1_7", "off_8_15", "off_ge16", "overlap"):
        assert total[bucket] > 0, bucket
    assert overlap17 == set(range(1, 17))
    assert max_chunks >= 3
    assert max_ops > 128  # two batches of the wave decoder (and > 64)
    assert ends_1byte_literal
    assert ends_copy
    # long back-references in the 16 KiB / 64 KiB geometry blocks
    assert max_offset > 32768


def test_corpus_directed_cases_all_present():
    job, cases = fc.directed_job()
    seen = set()
    for name, raw, ctype, payload in job.blocks():
        for o in fs.parse(payload)[1]:
            if o.kind == "copy":
                seen.add(o.offset)
    assert set(fs.DIRECTED_OFFSETS) <= seen
    # the tag-1 / tag-2 flip at the 2048 boundary
    forms = {}
    for name, raw, ctype, payload in job.blocks():
        for o in fs.parse(payload)[1]:
            if o.kind == "copy" and o.offset in (2047, 2048) and \
                    4 <= o.length <= 11:
                forms.setdefault(o.offset, set()).add(o.form)
    assert forms == {2047: {1}, 2048: {2}}


def test_corpus_geometry_has_far_offsets():
    for idx, geoms in enumerate(fc.GEOMETRY_JOBS):
        job = fc.geometry_job(idx)
        for (bs, ri, iri, codec), (_, _, rec) in zip(geoms, job.runs):
            if codec == "raw" or bs < 16384:
                continue
            far = max(o.offset for _, _, _, p in rec.blocks
                      for o in fs.parse(p)[1] if o.kind == "copy")
            assert far > 2048, (idx, bs)
            if bs == 65536:
                assert far > 32768, (idx, bs)
            # large blocks leave the LDS decoders for the global fallback
            assert any(fc.branch_of(t, len(p), len(r)) == "fallback"
                       for _, r, t, p in rec.blocks)


def test_project_codec_emits_none_of_this(corpus_blocks):
    """Why the corpus is needed: the project's own encoder, on the same
    blocks of up to 4 KiB, never emits a 4-byte-offset copy or a literal
    longer than 64 bytes, and never chunks a match: no op crosses one of its
    64 segment boundaries, so every copy is a whole match of at most one
    segment.  (A match that continues into the next segment shows up as a
    new same-offset copy cut at the boundary, never as snappy's
    64+64+..+60+rest pieces, which ignore the boundaries.)"""
    tag3 = long_literals = chunked = nblocks = 0
    for job, name, raw, ctype, payload in corpus_blocks:
        if len(raw) > 4096:
            continue
        ops = fs.parse(oracle.snappy_compress(raw))[1]
        nblocks += 1
        seg = max(16, (len(raw) + 63) // 64)
        tag3 += sum(o.kind == "copy" and o.form == 3 for o in ops)
        long_literals += sum(o.kind == "lit" and o.length > 64 for o in ops)
        dst = 0
        for o in ops:
            chunked += dst // seg != (dst + o.length - 1) // seg
            dst += o.length
    assert nblocks > 100
    assert (tag3, long_literals, chunked) == (0, 0, 0)
    # the foreign streams on the same blocks do all three
    crossing = 0
    for job, name, raw, ctype, payload in corpus_blocks:
        if len(raw) > 4096 or ctype == 0 or name == "dcw":
            continue
        seg = max(16, (len(raw) + 63) // 64)
        dst = 0
        for o in fs.parse(payload)[1]:
            crossing += dst // seg != (dst + o.length - 1) // seg
            dst += o.length
    assert crossing > 1000


def test_decmax_sizes_and_branches():
    job, plan = fc.decmax_job()
    blocks = job.runs[0][2].blocks
    assert len(blocks) == len(plan)  # one entry per block
    branches = {}
    for (label, policy, usize), (name, raw, ctype, payload) in zip(plan, blocks):
        assert len(raw) == usize, label
        if ctype:
            assert fs.read_preamble(payload)[0] == usize, label
        branches[label] = fc.branch_of(ctype, len(payload), usize)
    D = fc.DEC_MAX
    want = {
        "compressible_%d" % (D - 1): "lds",
        "compressible_%d" % D: "lds",
        "compressible_%d" % (D + 1): "fallback",  # usize > DEC_MAX, n small
        "compressible_6000": "fallback",
        "all_literal_%d" % (D - 6): "lds",  # n = DEC_MAX - 1
        "all_literal_%d" % (D - 5): "lds",  # n = DEC_MAX
        "all_literal_%d" % (D - 4): "fallback",  # n = DEC_MAX + 1
        "all_literal_%d" % (D - 1): "fallback",  # n > DEC_MAX >= usize
        "all_literal_%d" % D: "fallback",
        "fragmented_3500": "fallback",  # n > DEC_MAX through expansion
        "raw_4000": "raw",
        "raw_5003": "raw",
        "ends_on_copy": "lds",
    }
    assert branches == want
    by = {lab: blk for (lab, _, _), blk in zip(plan, blocks)}
    assert len(by["all_literal_%d" % (D - 5)][3]) == D
    assert len(by["fragmented_3500"][3]) > D
    assert len(by["compressible_%d" % (D + 1)][3]) < 1000


def test_malformed_inputs_fail_in_the_oracle():
    for name in fc.MALFORMED_NAMES + (fc.MALFORMED_FALLBACK,):
        sst, stream = fc.malformed_input(name)
        with pytest.raises(fs.SnappyError):
            fs.decode(stream)
        with pytest.raises(ValueError):
            oracle.read_sst(sst)


# ------------------------------------------------- the host decoder fuzzers
TOOL = os.path.join(REPO, "tools", "dec_host_fuzz")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None,
                               reason="g++ not installed")


def _build_host_tool(tmp_path, name):
    """`name`.cpp is compiled against the kernels' own dcw_snap_dec_lds.h
    (and the oracle codec).  -> executable path."""
    orc = os.path.join(REPO, "oracle")
    exe = tmp_path / name
    r = subprocess.run(
        ["g++", "-O2", "-I", os.path.join(REPO, "toplingdb_amd", "csrc"),
         "-o", str(exe),
         os.path.join(TOOL, name + ".cpp"),
         os.path.join(orc, "liborc.so"), "-Wl,-rpath," + orc],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


@needs_gxx
def test_host_decoder_fuzzers_build_and_pass(tmp_path):
    """dec_fuzz / wave_fuzz run the host build of snap_dec_lds (and a
    simulation of snap_dec_wave) against the oracle codec.  A kernel refactor
    that breaks the header's host build or the decoders' host behaviour
    fails here."""
    for name in ("dec_fuzz", "wave_fuzz"):
        r = subprocess.run([_build_host_tool(tmp_path, name)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "OK" in r.stdout


@needs_gxx
def test_kernel_decoders_on_foreign_corpus_host(tmp_path, corpus_blocks):
    """The kernels' own snap_dec_lds<0>/<1> source, compiled for the
    host, and the snap_dec_wave simulation decode every foreign stream of
    the corpus to the raw block and refuse every malformed stream."""
    recs = bytearray()
    n_good = n_bad = 0
    for job, name, raw, ctype, payload in corpus_blocks:
        if ctype == 0:
            continue
        recs += len(payload).to_bytes(4, "little")
        recs += len(raw).to_bytes(4, "little") + payload + raw
        n_good += 1
    some_raw = corpus_blocks[0][2]
    for s in fc.malformed_streams(some_raw).values():
        recs += len(s).to_bytes(4, "little") + b"\xff\xff\xff\xff" + s
        n_bad += 1
    path = tmp_path / "corpus.bin"
    path.write_bytes(bytes(recs))
    r = subprocess.run([_build_host_tool(tmp_path, "corpus_check"), str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "corpus check: %d streams (%d malformed), 0 failures" % (
        n_good + n_bad, n_bad) in r.stdout
