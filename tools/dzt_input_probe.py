"""DZT-input probe: what reading a DcwZipTable level costs, on one GPU.

  (a) BlockBasedTable run + DZT level run            -> DZT files
  (b) the same job, the DZT run replaced by its snappy
      BlockBasedTable twin (the comparison point; a build without DZT
      inputs can run it too)                          -> DZT files

16-byte keys, 100-byte values, two workloads: the benchmark's generated
values (a 50-byte random string twice: the DZT builder's dictionary table
is full of dict positions, finds nothing and stores these blocks RAW), and
"word" values made of 20-byte words from a small vocabulary, which the
sampled dictionary compresses (the dict-snappy decode path).  Both level
runs are written by the worker itself from one SST, so they hold the same
entries.  Prints one JSON line per job: ms_decode, the per-kernel times of the decode-side
kernels, the host parse time (with the DZT key-area checksum inside it) and
end-to-end input MB/s; the numbers vary run to run on a shared box.

Usage: python tools/dzt_input_probe.py [entries_per_run] [workdir]
"""
import ctypes
import json
import os
import re
import shutil
import sys
import tempfile

os.environ["DCW_PHASE_DEBUG"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402
import toplingdb_amd as dcw  # noqa: E402

DECODE_KERNELS = ("verify_checksum", "decompress", "count_entries",
                  "decode_entries", "decode_entries_g", "dzt_verify_vblocks",
                  "dzt_decompress", "dzt_decode_keys")


def run_job(lib, runs, outd, **kw):
    """-> (result, kernel stats, worker debug text) of the second of two runs
    (the first warms buffers and the page cache)."""
    for attempt in range(2):
        shutil.rmtree(outd, ignore_errors=True)
        os.makedirs(outd)
        lib.dcw_kernel_stats_reset()
        with tempfile.TemporaryFile() as cap:
            sys.stderr.flush()
            saved = os.dup(2)
            os.dup2(cap.fileno(), 2)
            try:
                res = dcw.execute(dcw.make_job(runs, outd, **kw))
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            cap.seek(0)
            text = cap.read().decode(errors="replace")
    buf = ctypes.create_string_buffer(16384)
    lib.dcw_kernel_stats_json(buf, 16384)
    return res, json.loads(buf.value.decode()), text


def word_sst(path, n, seed, seq_base):
    """n entries, 16-byte keys, 100-byte values of five 20-byte words."""
    import random
    rng = random.Random(99)
    words = [rng.randbytes(20) for _ in range(512)]
    rng = random.Random(seed)
    pick = rng.choices
    keys = sorted(rng.sample(range(10 ** 15), n))
    es = [(oracle.make_ikey(b"%016d" % k, seq_base + i, 1),
           b"".join(pick(words, k=5))) for i, k in enumerate(keys)]
    with open(path, "wb") as f:
        f.write(oracle.build_sst(es))


def dzt_block_mix(paths):
    """-> (raw blocks, dict-snappy blocks) over the DZT files."""
    import struct
    mix = [0, 0]
    for p in paths:
        with open(p, "rb") as f:
            d = f.read()
        _, value_off, _, vindex_off, props_off = struct.unpack_from(
            "<5Q", d, len(d) - 96)
        for o in range(vindex_off, props_off, 24):
            voff, csize = struct.unpack_from("<QI", d, o)
            mix[1 if d[value_off + voff + csize] == 2 else 0] += 1
    return mix


def report(tag, res, ks, text):
    def grab(pat):
        m = re.findall(pat, text)
        return float(m[-1]) if m else None
    print(json.dumps({
        "job": tag,
        "in_MB": round(res["in_bytes"] / 1e6, 1),
        "in_entries": res["in_entries"],
        "ms_decode": grab(r"ms_decode=([0-9.]+)"),
        "kernels_ms": {k: round(ks[k]["ms"], 3) for k in DECODE_KERNELS
                       if k in ks},
        "host_parse_ms": grab(r"parse=([0-9.]+)ms"),
        "host_dzt_keycsum_ms": grab(r"dzt_keycsum=([0-9.]+)ms"),
        "work_ms": round(res["work_time_usec"] / 1000.0, 1),
        "input_MBps": round(res["in_bytes"] / max(res["work_time_usec"], 1), 1),
    }), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_500_000
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="dzp_")
    os.makedirs(work, exist_ok=True)
    dcw.init(0)
    lib = dcw.lib()
    lib.dcw_kernel_stats_json.restype = ctypes.c_int32
    lib.dcw_kernel_stats_json.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    for workload in ("generated", "words"):
        one_workload(lib, workload, n, os.path.join(work, workload))
    dcw.shutdown()
    if len(sys.argv) <= 2:
        shutil.rmtree(work, ignore_errors=True)


def one_workload(lib, workload, n, work):
    os.makedirs(work, exist_ok=True)
    base = os.path.join(work, "level.sst")
    newer = os.path.join(work, "newer.sst")
    if workload == "generated":
        dcw.gen_sst(base, seed=1, num_entries=n, seq_base=1)
        dcw.gen_sst(newer, seed=2, num_entries=n, seq_base=1 + n)
    else:
        n = n // 2  # built entry by entry from Python
        word_sst(base, n, 1, 1)
        word_sst(newer, n, 2, 1 + n)
    level = {}
    for tag, otf in (("dzt", 1), ("bbt", 0)):
        outd = os.path.join(work, "level_" + tag)
        shutil.rmtree(outd, ignore_errors=True)
        os.makedirs(outd)
        r = dcw.execute(dcw.make_job([[base]], outd, compression=1,
                                     output_table_factory=otf))
        level[tag] = [f["path"] for f in r["files"]]
    raw, comp = dzt_block_mix(level["dzt"])
    print(json.dumps({"workload": workload, "dzt_level_value_blocks":
                      {"raw": raw, "dict_snappy": comp}}), flush=True)
    kw = dict(compression=1, output_table_factory=1)
    for tag, run in (("a_bbt+dzt_level", level["dzt"]),
                     ("b_bbt+bbt_twin_level", level["bbt"])):
        res, ks, text = run_job(lib, [[newer], run],
                                os.path.join(work, "out_" + tag[0]), **kw)
        report(workload + ":" + tag, res, ks, text)


if __name__ == "__main__":
    main()
