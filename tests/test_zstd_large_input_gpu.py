"""zstd input data blocks beyond the small decoder's staging size, decoded on
the GPU by k_decompress_zstd_large.

As tests/test_zstd_input_gpu_decode.py: every job is a bottommost compaction
whose inputs exist twice, with data blocks stored as type 7 by libzstd and as
raw twins.  The GPU reads the zstd files, the oracle the twins; the output
files must be identical byte for byte, and the kernel statistics must show
`decompress_zstd` on exactly the blocks within DEC_MAX and
`decompress_zstd_large` on exactly the larger ones without a content checksum.
tests/test_zstd_large_cpu.py runs the same frame kinds, and the malformed
frame used here, through the same decoder source on the CPU.
"""
import ctypes
import json
import os
import random
import sys

import pytest

import oracle
import toplingdb_amd as dcw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_corpus as fc  # noqa: E402
import foreign_lz4 as fl  # noqa: E402
import foreign_zstd as fz  # noqa: E402
import test_lz4_input_gpu as tl  # noqa: E402  (write, outdir, check)
import test_zstd_large_cpu as zl  # noqa: E402  (the CPU test's frames)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    dcw.init(0)
    yield
    dcw.shutdown()


def kernel_bytes():
    """-> alg_bytes of (decompress_zstd, decompress_zstd_large); None: no launch"""
    lib = dcw.lib()
    lib.dcw_kernel_stats_json.restype = ctypes.c_int32
    lib.dcw_kernel_stats_json.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    buf = ctypes.create_string_buffer(16384)
    lib.dcw_kernel_stats_json(buf, 16384)
    stats = json.loads(buf.value.decode())
    return tuple(stats[k]["alg_bytes"] if k in stats else None
                 for k in ("decompress_zstd", "decompress_zstd_large"))


def zstd_run(kvs, expect, level=1, checksum_every=0, **opts):
    """-> fl.build_pair's tuple; adds stored + decoded bytes of the blocks each
    kernel decodes to expect[0] (small) and expect[1] (large)."""
    def choose(i, raw):
        checksum = checksum_every and i % checksum_every == 0
        frame = fz.compress(raw, level, checksum=checksum)
        if not checksum:
            small = len(frame) <= fz.DEC_MAX and len(raw) <= fz.DEC_MAX
            expect[0 if small else 1] += len(fz.frame_block(frame, len(raw))) + len(raw)
        return fz.ZSTD, frame
    return fl.build_pair(kvs, choose, **opts)


def runs_kvs(seed, big_value=False):
    rng = random.Random(seed)
    kv0, kv1 = fc.two_runs(1500, 1100, rng, far=(30, 350))
    if big_value:  # one block of three zstd blocks among the 4 KiB ones
        kv0 = sorted(kv0 + [(fc.ukey(3), 70000, fc.TYPE_VALUE,
                             fz._record_text(200000, rng))])
    return kv0, kv1


# name -> (zstd_run arguments, tl.check arguments, environment)
CASES = {
    "block_16k_level1": (dict(block_size=16384, level=1), {}, {}),
    "block_64k_level19": (dict(block_size=65536, level=19), {}, {}),
    "big_value_among_4k": (dict(block_size=4096, big_value=True), {}, {}),
    "checksum_frames_stay_on_host": (dict(block_size=16384, checksum_every=3), {}, {}),
    "staged": (dict(block_size=16384), dict(staged=True), {}),
    "large_host_env": (dict(block_size=16384), {}, {"DCW_ZSTD_LARGE_HOST": "1"}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_large_frames(tmp_path, monkeypatch, name):
    run_kw, check_kw, env = CASES[name]
    run_kw = dict(run_kw)
    expect = [0, 0]
    kvs = runs_kvs(0x90 + sorted(CASES).index(name), run_kw.pop("big_value", False))
    job = [zstd_run(kv, expect, **run_kw) for kv in kvs]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dcw.lib().dcw_kernel_stats_reset()
    tl.check(tmp_path, job, **check_kw)
    assert expect[1] > 0 and (expect[0] > 0 or not run_kw.get("block_size") == 4096)
    # a kernel without blocks is not launched; with DCW_ZSTD_LARGE_HOST the
    # large ones took the host path
    assert kernel_bytes() == (expect[0] or None, None if env else expect[1])


def test_malformed_large_frame_refused(tmp_path):
    """A bounds decision, not a fault: refused with no output, and the worker
    runs a good job right after.  libzstd refuses the frame, and
    tools/zstd_large_host has refused it sanitizer-clean."""
    (payload,) = [p for n, p, want in zl.mutations(zl.large_frames())
                  if n == "text_16384_l1.flip@2289" and want is None]
    kv0, kv1 = runs_kvs(0x9F)
    count = [0]

    def codec(raw):
        count[0] += 1
        if count[0] == 2:
            return fz.ZSTD, payload
        return fz.ZSTD, fz.frame_block(fz.compress(raw), len(raw))

    entries = [(oracle.make_ikey(k, s, t), v) for k, s, t, v in kv0]
    p = tl.write(tmp_path, "bad.sst", oracle.build_sst(
        entries, oracle.default_table_opts(block_size=16384),
        data_block_codec=codec))
    assert count[0] >= 3
    out = tl.outdir(tmp_path, "bad_out")
    with pytest.raises(RuntimeError):
        dcw.execute(dcw.make_job([[p]], out, bottommost_level=1))
    assert os.listdir(out) == []
    tl.check(tmp_path, [zstd_run(kv, [0, 0], block_size=16384) for kv in (kv0, kv1)])
