"""DcwZipTable files as compaction INPUTS on the GPU.

Parity without touching the oracle: a compaction's output depends only on
the entry streams and the job descriptor, so for each DZT input F the test
builds its BlockBasedTable twin, oracle.build_sst(oracle.dzt_read(F)), and
the worker's outputs for the job with DZT inputs must be byte-identical to
oracle.execute on the same job with the twins (files, smallest/largest,
seqnos, out_entries; in_bytes differs by construction).  DZT inputs are
made on the CPU by oracle.execute(..., output_table_factory=1)."""
import concurrent.futures
import ctypes
import json
import os
import random
import sys

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dzt_foreign as zf  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    dcw.init(0)
    yield
    dcw.shutdown()


# ------------------------------------------------------------------ helpers
def ukey(i, width=16, prefix=b"k"):
    return prefix + zf.ukey(i, width)[1:]


def puts(n, value, seq0=1000, width=16, step=1, prefix=b"k"):
    """n Put entries; value: bytes or callable(i) -> bytes."""
    vf = value if callable(value) else (lambda i: value)
    return [(oracle.make_ikey(ukey(i * step, width, prefix), seq0 + i, 1),
             vf(i)) for i in range(n)]


def write_sst(tmp, name, entries, **opts):
    p = os.path.join(str(tmp), name)
    with open(p, "wb") as f:
        f.write(oracle.build_sst(entries, oracle.default_table_opts(**opts)))
    return p


def is_dzt(path):
    with open(path, "rb") as f:
        return f.read()[-8:] == b"DCWZIP01"


def twins(tmp, runs):
    """The same runs with every DZT file replaced by its twin."""
    out = []
    for r, files in enumerate(runs):
        tr = []
        for i, p in enumerate(files):
            if is_dzt(p):
                t = os.path.join(str(tmp), "twin_%d_%d_%s.sst" % (
                    r, i, os.path.basename(os.path.dirname(p))))
                with open(t, "wb") as f:
                    f.write(zf.twin_sst(p))
                p = t
            tr.append(p)
        out.append(tr)
    return out


def fresh(tmp, name):
    d = os.path.join(str(tmp), name)
    n = 0
    while os.path.exists(d + str(n)):
        n += 1
    os.makedirs(d + str(n))
    return d + str(n)


def same_outputs(rg, ro):
    assert rg["out_entries"] == ro["out_entries"]
    assert len(rg["files"]) == len(ro["files"])
    for fg, fo in zip(rg["files"], ro["files"]):
        with open(fg["path"], "rb") as a, open(fo["path"], "rb") as b:
            da, db = a.read(), b.read()
        assert da == db, "%s differs from the oracle's (%d vs %d bytes)" % (
            fg["path"], len(da), len(db))
        for k in ("smallest", "largest", "smallest_seqno", "largest_seqno",
                  "num_entries"):
            assert fg[k] == fo[k], k


def parity(tmp, runs, **kw):
    assert any(is_dzt(p) for files in runs for p in files)
    ro = oracle.execute(oracle.make_job(twins(tmp, runs), fresh(tmp, "orc"),
                                        **kw))
    rg = dcw.execute(dcw.make_job(runs, fresh(tmp, "gpu"), **kw))
    same_outputs(rg, ro)
    return rg


def kernel_names():
    lib = dcw.lib()
    lib.dcw_kernel_stats_json.restype = ctypes.c_int32
    lib.dcw_kernel_stats_json.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    buf = ctypes.create_string_buffer(16384)
    lib.dcw_kernel_stats_json(buf, 16384)
    return set(json.loads(buf.value.decode()))


DZT_KERNELS = {"dzt_verify_vblocks", "dzt_decompress", "dzt_decode_keys"}


# ------------------------------------------------------------- entry counts
COUNTS = (1, 63, 64, 65, 255, 256, 257, 5000)


@pytest.fixture(scope="module")
def count_inputs(tmp_path_factory):
    """n -> (DZT level run, overlapping newer BlockBasedTable run)."""
    tmp = tmp_path_factory.mktemp("counts")
    rng = random.Random(3)
    out = {}
    for n in COUNTS:
        es = puts(n, lambda i: rng.randbytes(20) + b"v%07d" % i * 8, step=2)
        kw = dict(target_file_size=150_000) if n == 5000 else {}
        run = zf.oracle_dzt(tmp, "c%d" % n, es, **kw)
        if n == 5000:
            assert len(run) >= 3  # one level run of several DZT files
            z = zf.Dzt(open(run[0], "rb").read())
            assert len(z.kblocks) > 2 and len(z.vblocks) > 2
        newer = puts((n + 2) // 3, b"newer" * 7, seq0=900_000, step=3)
        out[n] = (run, write_sst(tmp, "newer%d.sst" % n, newer))
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_entry_counts_single_run(tmp_path, count_inputs, n):
    run, _ = count_inputs[n]
    rg = parity(tmp_path, [run], compression=1)
    assert rg["out_entries"] == n


@pytest.mark.parametrize("n", COUNTS)
def test_entry_counts_merged_with_bbt(tmp_path, count_inputs, n):
    run, newer = count_inputs[n]
    parity(tmp_path, [[newer], run], compression=1)


def test_mixed_kinds_inside_one_run(tmp_path, count_inputs):
    """A level run of a BlockBasedTable file, a DZT file and another
    BlockBasedTable file, in key order, under a newer run."""
    run, newer = count_inputs[257]
    lo = write_sst(tmp_path, "lo.sst", puts(100, b"lo" * 30, seq0=10,
                                            prefix=b"a"))
    hi = write_sst(tmp_path, "hi.sst", puts(100, b"hi" * 30, seq0=200,
                                            prefix=b"z"))
    parity(tmp_path, [[newer], [lo] + run + [hi]], compression=1)
    parity(tmp_path, [[lo] + run, [newer]], compression=0)


# ------------------------------------------------------------------- values
def _value_fn(kind):
    rng = random.Random(7)
    return {
        "empty": (300, lambda i: b""),
        "b100": (300, lambda i: rng.randbytes(30) + b"%070d" % i),
        "b9000": (24, lambda i: (b"%09d-" % i) * 900),
        "b20000_incompressible": (6, lambda i: rng.randbytes(20000)),
        "b20000_compressible": (6, lambda i: (b"%07d" % i + b"abcdefghi") * 1250),
    }[kind]


@pytest.mark.parametrize("compression", (1, 0))
@pytest.mark.parametrize("kind", ("empty", "b100", "b9000",
                                  "b20000_incompressible",
                                  "b20000_compressible"))
def test_value_shapes(tmp_path, kind, compression):
    n, vf = _value_fn(kind)
    run = zf.oracle_dzt(tmp_path, "v", puts(n, vf), compression=compression)
    z = zf.Dzt(open(run[0], "rb").read())
    btypes = {b[0] for b in z.vblocks}
    ulens = [b[2] for b in z.vblocks]
    if compression == 0 or kind == "b20000_incompressible":
        assert btypes == {0}
    elif kind != "empty":
        assert btypes == {2}
    if kind == "b9000":
        assert max(ulens) == 9000 and len(ulens) == n  # 16384 B rule closes
    if kind.startswith("b20000"):
        assert ulens == [20000] * n  # own block, over the LDS bound
    newer = write_sst(tmp_path, "n.sst", puts(n // 2, b"x" * 50, seq0=90_000,
                                              step=2))
    # (a 20 KB data block is outside the worker's snappy OUTPUT envelope)
    out_comp = 0 if kind.startswith("b20000") else 1
    parity(tmp_path, [run], compression=out_comp)
    parity(tmp_path, [[newer], run], compression=compression and out_comp)


# --------------------------------------------------------------- tombstones
@pytest.fixture(scope="module")
def tombstone_inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tomb")
    newer, older = [], []
    for i in range(400):
        k = ukey(i)
        older.append((oracle.make_ikey(k, 100 + i, 1), b"old%05d" % i * 9))
        if i % 5 == 0:
            newer.append((oracle.make_ikey(k, 5000 + i, 0), b""))  # Delete
        elif i % 5 == 1:
            newer.append((oracle.make_ikey(k, 5000 + i, 7), b""))  # SingleDelete
        elif i % 5 == 2:
            newer.append((oracle.make_ikey(k, 5000 + i, 1), b"new%05d" % i * 9))
    # not bottommost, a file below that may hold the keys, and a snapshot
    # under every entry: nothing may drop the tombstones
    run = zf.oracle_dzt(tmp, "tomb", newer, bottommost_level=0,
                        levels_below=[[(b"a", b"z", 1000)]], snapshots=[50],
                        earliest_write_conflict_snapshot=50)
    got = oracle.dzt_read(open(run[0], "rb").read())
    types = [ik[-8] for ik, _ in got]
    assert types.count(0) == 80 and types.count(7) == 80
    return run, write_sst(tmp, "older.sst", older)


@pytest.mark.parametrize("snapshots", ([], [5100]))
@pytest.mark.parametrize("bottommost", (1, 0))
def test_tombstones_in_dzt_input(tmp_path, tombstone_inputs, bottommost,
                                 snapshots):
    run, older = tombstone_inputs
    kw = dict(bottommost_level=bottommost, compression=1)
    if not bottommost:  # tombstones that meet nothing stay in the output
        kw.update(levels_below=[[(b"a", b"z", 1000)]])
    if snapshots:
        kw.update(snapshots=snapshots,
                  earliest_write_conflict_snapshot=snapshots[0])
    parity(tmp_path, [run, [older]], **kw)
    parity(tmp_path, [run], **kw)


# ----------------------------------------------------------- output formats
def test_dzt_inputs_to_dzt_output(tmp_path, count_inputs):
    """The steady-state L2->L3 shape: one BlockBasedTable run + one DZT
    level run -> DZT files, bit-exact."""
    run, newer = count_inputs[5000]
    rg = parity(tmp_path, [[newer], run], compression=1,
                output_table_factory=1, target_file_size=200_000)
    assert len(rg["files"]) >= 2 and all(is_dzt(f["path"]) for f in rg["files"])
    assert kernel_names() >= DZT_KERNELS


@pytest.mark.parametrize("ct", (1, 4))
def test_checksum_types(tmp_path, ct):
    run = zf.oracle_dzt(tmp_path, "ct", puts(300, lambda i: b"%0100d" % i),
                        checksum_type=ct)
    assert zf.Dzt(open(run[0], "rb").read()).ct == ct
    newer = write_sst(tmp_path, "n.sst", puts(90, b"n" * 40, seq0=70_000, step=3),
                      checksum_type=ct)
    parity(tmp_path, [[newer], run], compression=1, checksum_type=ct)


def test_mixed_checksum_types_refused(tmp_path):
    run = zf.oracle_dzt(tmp_path, "ct", puts(50, b"v" * 30), checksum_type=1)
    other = write_sst(tmp_path, "n.sst", puts(50, b"n" * 40, seq0=70_000),
                      checksum_type=4)
    with pytest.raises(RuntimeError, match="mixed input checksum"):
        dcw.execute(dcw.make_job([[other], run], fresh(tmp_path, "gpu")))


# ------------------------------------------------------------- general mode
@pytest.mark.parametrize("U", (24, 48))
def test_general_key_mode(tmp_path, U):
    run = zf.oracle_dzt(tmp_path, "g", puts(300, lambda i: b"%060d" % i,
                                            width=U))
    assert zf.Dzt(open(run[0], "rb").read()).U == U
    rng = random.Random(U)
    mixed = sorted({(b"k%0" + str(rng.randint(3, 40)).encode() + b"d")
                    % rng.randrange(10 ** 3) for _ in range(200)})
    bbt = write_sst(tmp_path, "mixed.sst",
                    [(oracle.make_ikey(k, 80_000 + i, 1), b"m%d" % i)
                     for i, k in enumerate(mixed)])
    parity(tmp_path, [[bbt], run], compression=1)


def test_uniform_bbt_of_another_length_goes_general(tmp_path):
    run = zf.oracle_dzt(tmp_path, "g", puts(100, b"v" * 40, width=16))
    bbt = write_sst(tmp_path, "u8.sst", puts(100, b"w" * 40, seq0=50_000,
                                             width=8))
    parity(tmp_path, [[bbt], run], compression=1)


def test_user_key_56_refused(tmp_path):
    run = zf.oracle_dzt(tmp_path, "g", puts(40, b"v" * 40, width=56))
    out = fresh(tmp_path, "gpu")
    with pytest.raises(RuntimeError, match="48 B"):
        dcw.execute(dcw.make_job([run], out))
    assert os.listdir(out) == []


# ------------------------------------------------------ staged path, pooling
def test_staged_mixed_job_matches_unstaged(tmp_path, count_inputs):
    run, newer = count_inputs[5000]
    runs = [[newer], run]
    r1 = dcw.execute(dcw.make_job(runs, fresh(tmp_path, "a"), compression=1))
    jd = dcw.make_job(runs, fresh(tmp_path, "b"), compression=1)
    h = dcw.stage_inputs(jd)
    jd.staged_handle = h
    r2 = dcw.execute(jd)
    r3 = dcw.execute(jd)  # the staged tables survive a job
    dcw.release_staged(h)
    same_outputs(r2, r1)
    same_outputs(r3, r1)
    assert r2["in_bytes"] == r1["in_bytes"] == sum(
        os.path.getsize(p) for files in runs for p in files)


def test_pool_reuse_and_concurrency(tmp_path, count_inputs):
    run, newer = count_inputs[5000]
    small, small_newer = count_inputs[65]
    bbt_runs = [[newer], [write_sst(tmp_path, "b.sst", puts(3000, b"b" * 90))]]
    want_bbt = oracle.execute(oracle.make_job(bbt_runs, fresh(tmp_path, "ob"),
                                              compression=1))
    dcw.lib().dcw_kernel_stats_reset()
    same_outputs(dcw.execute(dcw.make_job(bbt_runs, fresh(tmp_path, "gb"),
                                          compression=1)), want_bbt)
    # no DZT input: the kernel sequence of before, nothing of the DZT branch
    names = kernel_names()
    assert not names & DZT_KERNELS
    assert {"verify_checksum", "decompress", "count_entries",
            "decode_entries"} <= names
    for _ in range(2):  # alternate on the pooled job objects
        parity(tmp_path, [[newer], run], compression=1)
        same_outputs(dcw.execute(dcw.make_job(bbt_runs, fresh(tmp_path, "gb"),
                                              compression=1)), want_bbt)
        parity(tmp_path, [[small_newer], small], compression=1)
    assert kernel_names() >= DZT_KERNELS
    want_dzt = oracle.execute(oracle.make_job(
        twins(tmp_path, [[newer], run]), fresh(tmp_path, "oz"), compression=1))
    with concurrent.futures.ThreadPoolExecutor(2) as ex:
        fz = ex.submit(dcw.execute, dcw.make_job(
            [[newer], run], fresh(tmp_path, "cz"), compression=1))
        fb = ex.submit(dcw.execute, dcw.make_job(
            bbt_runs, fresh(tmp_path, "cb"), compression=1))
        same_outputs(fz.result(), want_dzt)
        same_outputs(fb.result(), want_bbt)


# ---------------------------------------------------------- foreign streams
@pytest.fixture(scope="module")
def foreign(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("foreign")
    path, d = zf.foreign_file(tmp)
    data = open(path, "rb").read()
    good_runs = [[write_sst(tmp, "fn.sst", puts(200, b"f" * 33, seq0=600_000,
                                                step=3))], [path]]
    want = oracle.execute(oracle.make_job(twins(tmp, good_runs),
                                          fresh(tmp, "orc"), compression=1))
    return tmp, data, d, good_runs, want


@pytest.mark.parametrize("mode", zf.MODES)
def test_foreign_streams(tmp_path, foreign, mode):
    """Value blocks re-encoded by the helper's encoder against a dictionary
    the test chooses; test_dzt_input_cpu.py asserts on the CPU that these
    very files hold every op class the decoder must accept."""
    _, data, d, good_runs, want = foreign
    p = os.path.join(fresh(tmp_path, "in"), "foreign.dzt")
    with open(p, "wb") as f:
        f.write(zf.rewrite(data, zf.encoder(mode), d))
    rg = dcw.execute(dcw.make_job([good_runs[0], [p]], fresh(tmp_path, "gpu"),
                                  compression=1))
    same_outputs(rg, want)  # same entries as the original file
    parity(tmp_path, [[p]], compression=0)


# --------------------------------------------------------- malformed inputs
@pytest.mark.parametrize("name", zf.MALFORMED)
def test_malformed_inputs_refused(tmp_path, foreign, name):
    """Each is caught by a check in parse_dzt, dzt_snap_dec, dzt_key_next or
    the DZT kernels; the worker then runs a good job bit-exact."""
    _, data, _, good_runs, want = foreign
    p = os.path.join(fresh(tmp_path, "in"), "bad.dzt")
    with open(p, "wb") as f:
        f.write(zf.malformed(data, name))
    out = fresh(tmp_path, "gpu")
    with pytest.raises(RuntimeError):
        dcw.execute(dcw.make_job([good_runs[0], [p]], out, compression=1))
    assert os.listdir(out) == []
    same_outputs(dcw.execute(dcw.make_job(good_runs, fresh(tmp_path, "ok"),
                                          compression=1)), want)


def test_zstd_bbt_with_dzt_refused_cleanly(tmp_path, foreign):
    _, _, _, good_runs, _ = foreign
    zstd = write_sst(tmp_path, "z.sst", puts(300, b"z" * 80, seq0=800_000),
                     compression=7)
    out = fresh(tmp_path, "gpu")
    with pytest.raises(RuntimeError, match="zstd"):
        dcw.execute(dcw.make_job([[zstd], good_runs[1]], out, compression=1))
    assert os.listdir(out) == []
