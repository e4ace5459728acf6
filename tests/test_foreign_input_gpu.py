"""GPU decode side on inputs the worker did not write itself: data blocks
coded by foreign snappy encoders (tests/foreign_snappy.py), block sizes on
both sides of the LDS decoders' DEC_MAX, non-default input table geometry,
every decoder variant, and clean refusal of malformed streams.

Every job is a bottommost compaction of 2 runs with uncompressed output.
Each is checked twice, both exactly: the output files are bit-identical to
the oracle's on the same inputs, and reading them back gives the survivor
list computed in plain Python from the known KVs (so a misreading shared by
the oracle and the GPU cannot pass).  tests/test_foreign_input_cpu.py
asserts, on the CPU, that this corpus contains the op forms it is here for.
"""
import json
import os
import subprocess
import sys

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_corpus as fc  # noqa: E402
import foreign_snappy as fs  # noqa: E402

pytestmark = pytest.mark.gpu

JOB_KW = dict(compression=0, bottommost_level=1)
RUNNER = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "foreign_variant_runner.py")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    dcw.init(0)
    yield
    dcw.shutdown()


def assert_identical(rg, ro):
    assert rg["out_entries"] == ro["out_entries"]
    assert len(rg["files"]) == len(ro["files"])
    for fg, fo in zip(rg["files"], ro["files"]):
        assert fg["file_number"] == fo["file_number"]
        with open(fg["path"], "rb") as a, open(fo["path"], "rb") as b:
            da, db = a.read(), b.read()
        assert da == db, "GPU SST %s differs from oracle (sizes %d vs %d)" % (
            fg["path"], len(da), len(db))
        for field in ("smallest", "largest", "smallest_seqno", "largest_seqno"):
            assert fg[field] == fo[field], field


def assert_survivors(files, job):
    got = []
    for f in files:
        with open(f["path"], "rb") as fh:
            got += oracle.read_sst(fh.read())
    assert got == job.expected


def oracle_run(directory, job):
    """-> (runs argument, oracle result); the inputs land in `directory`."""
    runs = job.write_inputs(directory)
    out = os.path.join(str(directory), job.name + "_orc")
    os.makedirs(out)
    return runs, oracle.execute(oracle.make_job(runs, out, **JOB_KW))


def run_and_check(tmp_path, job):
    runs, ro = oracle_run(tmp_path, job)
    out = tmp_path / (job.name + "_gpu")
    out.mkdir()
    rg = dcw.execute(dcw.make_job(runs, str(out), **JOB_KW))
    assert_identical(rg, ro)
    assert_survivors(rg["files"], job)
    assert rg["out_entries"] == len(job.expected)


# ---- a. foreign streams, default decoder ----
@pytest.mark.parametrize("policy", sorted(fs.POLICIES))
def test_foreign_policy(tmp_path, policy):
    run_and_check(tmp_path, fc.policy_job(policy))


def test_directed_offset_length_sweep(tmp_path):
    run_and_check(tmp_path, fc.directed_job()[0])


def test_mixed_raw_project_foreign_blocks(tmp_path):
    job = fc.mixed_job()
    assert {b[0] for b in job.blocks()} >= {"raw", "dcw", "greedy",
                                            "fragmented", "all_literal"}
    run_and_check(tmp_path, job)


# ---- b. DEC_MAX boundary ----
def test_dec_max_boundary(tmp_path):
    job, plan = fc.decmax_job()
    taken = {}
    for (label, _, usize), (_, raw, ctype, payload) in zip(
            plan, job.runs[0][2].blocks):
        if ctype:  # the size the kernel will read from the stream itself
            assert fs.read_preamble(payload)[0] == usize == len(raw)
        taken[label] = (fc.branch_of(ctype, len(payload), len(raw)),
                        len(payload), len(raw))
    print("k_decompress branch per block (branch, n, usize):", taken)
    assert {t[0] for t in taken.values()} == {"raw", "lds", "fallback"}
    D = fc.DEC_MAX
    assert taken["compressible_%d" % D][0] == "lds"
    assert taken["compressible_%d" % (D + 1)][0] == "fallback"
    assert taken["all_literal_%d" % (D - 5)][:2] == ("lds", D)
    assert taken["all_literal_%d" % (D - 4)][:2] == ("fallback", D + 1)
    assert taken["fragmented_3500"][0] == "fallback"
    run_and_check(tmp_path, job)


# ---- c. foreign geometry ----
@pytest.mark.parametrize("idx", range(len(fc.GEOMETRY_JOBS)))
def test_foreign_geometry(tmp_path, idx):
    run_and_check(tmp_path, fc.geometry_job(idx))


# ---- d. decoder variants, one fresh child process each ----
VARIANTS = (("DCW_DEC_PIPE", "0"), ("DCW_DEC_PIPE", "1"),
            ("DCW_DEC_PIPE", "2"), ("DCW_DECOMP_V", "1"),
            ("DCW_DECOMP_V", "2"))
CHILD_TIMEOUT_S = 120
_child_died = []  # once a child dies no further child is started


@pytest.fixture(scope="module")
def variant_inputs(tmp_path_factory):
    """Corpus (a) + (b) written once, with the oracle's outputs."""
    d = tmp_path_factory.mktemp("variants")
    return {job.name: (job,) + oracle_run(d, job)
            for job in fc.decoder_jobs()}


@pytest.mark.parametrize("var,val", VARIANTS,
                         ids=["%s=%s" % v for v in VARIANTS])
def test_decoder_variant(tmp_path, variant_inputs, var, val):
    if _child_died:
        pytest.skip("an earlier decoder-variant child died: " + _child_died[0])
    manifest = {"result": str(tmp_path / "result.json"), "jobs": []}
    for name, (job, runs, ro) in variant_inputs.items():
        manifest["jobs"].append(dict(name=name, runs=runs, kw=JOB_KW,
                                     out_dir=str(tmp_path / (name + "_gpu"))))
    mpath = tmp_path / "manifest.json"
    mpath.write_text(json.dumps(manifest))
    env = {k: v for k, v in os.environ.items()
           if k not in ("DCW_DEC_PIPE", "DCW_DECOMP_V")}
    env[var] = val
    try:
        r = subprocess.run([sys.executable, RUNNER, str(mpath)], env=env,
                           capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _child_died.append("%s=%s timed out" % (var, val))
        pytest.fail(_child_died[0])
    if r.returncode != 0:
        _child_died.append("%s=%s exited %d" % (var, val, r.returncode))
        pytest.fail(_child_died[0] + "\n" + r.stdout[-2000:] + r.stderr[-4000:])
    with open(manifest["result"]) as f:
        results = json.load(f)
    errors = {n: x["error"] for n, x in results.items() if "error" in x}
    if errors:
        _child_died.append("%s=%s job failed: %r" % (var, val, errors))
        pytest.fail(_child_died[0])
    assert set(results) == set(variant_inputs)
    for name, (job, runs, ro) in variant_inputs.items():
        rg = results[name]
        assert rg["out_entries"] == ro["out_entries"], name
        assert len(rg["files"]) == len(ro["files"]), name
        for fg, fo in zip(rg["files"], ro["files"]):
            assert fg["file_number"] == fo["file_number"]
            with open(fg["path"], "rb") as a, open(fo["path"], "rb") as b:
                assert a.read() == b.read(), (name, fg["path"])
        assert_survivors(rg["files"], job)


# ---- e. rejection parity (default decoder, in-process) ----
@pytest.fixture(scope="module")
def good_job(tmp_path_factory):
    d = tmp_path_factory.mktemp("good")
    job = fc.good_small_job()
    return (job,) + oracle_run(d, job)


@pytest.mark.parametrize("name", fc.MALFORMED_NAMES + (fc.MALFORMED_FALLBACK,))
def test_malformed_stream_refused(tmp_path, good_job, name):
    sst, stream = fc.malformed_input(name)
    with pytest.raises(fs.SnappyError):
        fs.decode(stream)
    with pytest.raises(ValueError):
        oracle.read_sst(sst)
    usize_known = name != "varint_6_bytes"
    if usize_known:
        n, usize = len(stream), fs.read_preamble(stream)[0]
        want = "fallback" if name == fc.MALFORMED_FALLBACK else "lds"
        assert fc.branch_of(1, n, usize) == want
    p = tmp_path / "bad.sst"
    p.write_bytes(sst)
    out = tmp_path / "bad_out"
    out.mkdir()
    with pytest.raises(RuntimeError):
        dcw.execute(dcw.make_job([[str(p)]], str(out), **JOB_KW))
    assert os.listdir(out) == []
    # the process still runs a good job correctly
    job, runs, ro = good_job
    out2 = tmp_path / "good_out"
    out2.mkdir()
    rg = dcw.execute(dcw.make_job(runs, str(out2), **JOB_KW))
    assert_identical(rg, ro)
    assert_survivors(rg["files"], job)
