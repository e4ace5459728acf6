"""LZ4-output probe: what encoding LZ4 output blocks costs next to snappy, on
one GPU.

The benchmark's 8-way workload (bench.py: 8 generated snappy runs, 16-byte
keys, target_file_size 64 MiB, bottommost), run twice over the same inputs:
  (snappy) compression=1: k_compress
  (lz4)    compression=4: k_compress_lz4
Jobs run one at a time; the second of two executions is reported.  Prints
one JSON line per job: the encoder's total time, its microseconds per
uncompressed MB (the kernel statistics keep 1.6 x resp. 2.6 x the
uncompressed bytes as algorithmic bytes), output bytes, and at the end the
two ratios lz4/snappy.  Only the figures of one run compare: boxes vary
15-25 % run to run.

Usage: python tools/lz4_output_probe.py [entries_per_run] [workdir]
"""
import ctypes
import json
import os
import shutil
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toplingdb_amd as dcw  # noqa: E402

ENCODERS = {1: ("compress", 1.6), 4: ("compress_lz4", 2.6)}


def run_job(lib, runs, outd, compression):
    for _ in range(2):  # the first warms buffers and the page cache
        shutil.rmtree(outd, ignore_errors=True)
        os.makedirs(outd)
        lib.dcw_kernel_stats_reset()
        res = dcw.execute(dcw.make_job(runs, outd, compression=compression,
                                       target_file_size=64 << 20,
                                       bottommost_level=1))
    buf = ctypes.create_string_buffer(16384)
    lib.dcw_kernel_stats_json(buf, 16384)
    return res, json.loads(buf.value.decode())


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 920_000
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="l4o_")
    os.makedirs(work, exist_ok=True)
    dcw.init(0)
    lib = dcw.lib()
    lib.dcw_kernel_stats_json.restype = ctypes.c_int32
    lib.dcw_kernel_stats_json.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    runs = []
    for r in range(8):
        p = os.path.join(work, "in%d.sst" % r)
        dcw.gen_sst(p, seed=0x746F706C696E6721 + r, num_entries=n,
                    seq_base=1 + r * n, compression=1)
        runs.append([p])
    seen = {}
    for compression, (kernel, factor) in sorted(ENCODERS.items()):
        res, ks = run_job(lib, runs, os.path.join(work, "out%d" % compression),
                          compression)
        k = ks[kernel]
        unc_mb = k["alg_bytes"] / factor / 1e6
        seen[compression] = (1000 * k["ms"] / unc_mb, res["out_bytes"])
        print(json.dumps({
            "job": "8 x %d entries, compression=%d" % (n, compression),
            "encoder": kernel,
            "launches": k["launches"],
            "encoder_ms": round(k["ms"], 3),
            "uncompressed_MB": round(unc_mb, 1),
            "us_per_uncompressed_MB": round(seen[compression][0], 2),
            "emit_side_ms": {x: round(ks[x]["ms"], 3)
                             for x in ("emit", "checksum", "pack") if x in ks},
            "out_MB": round(res["out_bytes"] / 1e6, 1),
            "work_ms": round(res["work_time_usec"] / 1000.0, 1),
            "input_MBps": round(res["in_bytes"] / max(res["work_time_usec"], 1), 1),
        }), flush=True)
    print(json.dumps({
        "lz4_over_snappy_time_per_MB": round(seen[4][0] / seen[1][0], 2),
        "lz4_over_snappy_out_bytes": round(seen[4][1] / seen[1][1], 3),
    }), flush=True)
    dcw.shutdown()
    if len(sys.argv) <= 2:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
