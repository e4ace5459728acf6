"""Large-block probe: what snappy output costs when every data block is over
16 KiB (k_compress_large) next to the default kernel, on one GPU.

One named job, run twice over the same two input runs of 1 KiB values:
  (large)   block_size=65536: every block goes to k_compress_large
  (default) block_size=4096:  every block goes to k_compress
Values are half random, half one shared 23-byte period, so blocks of either
size pass the 87.5 % ratio test and pass 2 of the large kernel runs.  The
jobs run one at a time (jobs-in-flight 1).  Prints one JSON line per job:
per-launch time and algorithmic bytes per ms (1.6 x uncompressed bytes, the
figure `dcw_kernel_stats_json` keeps) of the compress kernels, the stored
ratio and end-to-end input MB/s; the second of two executions is reported.
The numbers vary run to run on a shared box.

Usage: python tools/big_block_probe.py [entries_per_run] [workdir]
"""
import ctypes
import json
import os
import random
import shutil
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402
import toplingdb_amd as dcw  # noqa: E402

KERNELS = ("emit", "compress", "compress_large", "checksum", "pack")


def kib_sst(path, n, seed, seq_base):
    """n entries, 16-byte keys, 1 KiB values: 512 random bytes and 512 of a
    period shared by every value."""
    pat = (random.Random(23).randbytes(23) * 23)[:512]
    rng = random.Random(seed)
    keys = sorted(rng.sample(range(10 ** 15), n))
    es = [(oracle.make_ikey(b"%016d" % k, seq_base + i, 1),
           rng.randbytes(512) + pat) for i, k in enumerate(keys)]
    with open(path, "wb") as f:
        f.write(oracle.build_sst(es))


def run_job(lib, runs, outd, **kw):
    for _ in range(2):  # the first warms buffers and the page cache
        shutil.rmtree(outd, ignore_errors=True)
        os.makedirs(outd)
        lib.dcw_kernel_stats_reset()
        res = dcw.execute(dcw.make_job(runs, outd, **kw))
    buf = ctypes.create_string_buffer(16384)
    lib.dcw_kernel_stats_json(buf, 16384)
    return res, json.loads(buf.value.decode())


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="bbp_")
    os.makedirs(work, exist_ok=True)
    dcw.init(0)
    lib = dcw.lib()
    lib.dcw_kernel_stats_json.restype = ctypes.c_int32
    lib.dcw_kernel_stats_json.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    runs = []
    for r in range(2):
        p = os.path.join(work, "in%d.sst" % r)
        kib_sst(p, n, 1 + r, 1 + r * n)
        runs.append([p])
    for tag, bs in (("large", 65536), ("default", 4096)):
        res, ks = run_job(lib, runs, os.path.join(work, "out_" + tag),
                          compression=1, bottommost_level=1, block_size=bs)
        kern = {}
        for k in KERNELS:
            if k in ks and ks[k]["launches"]:
                ms = ks[k]["ms"] / ks[k]["launches"]
                kern[k] = {"launches": ks[k]["launches"],
                           "ms_per_launch": round(ms, 3),
                           "alg_MB_per_ms": round(
                               ks[k]["alg_bytes"] / ks[k]["launches"] / 1e6 /
                               max(ms, 1e-9), 1)}
        print(json.dumps({
            "job": "2x%d entries, 1 KiB values, block_size=%d (%s)" % (n, bs, tag),
            "in_MB": round(res["in_bytes"] / 1e6, 1),
            "out_MB": round(res["out_bytes"] / 1e6, 1),
            "out_entries": res["out_entries"],
            "files": len(res["files"]),
            "kernels": kern,
            "work_ms": round(res["work_time_usec"] / 1000.0, 1),
            "input_MBps": round(res["in_bytes"] / max(res["work_time_usec"], 1), 1),
        }), flush=True)
    dcw.shutdown()
    if len(sys.argv) <= 2:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
