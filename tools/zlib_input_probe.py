"""zlib-input probe: what decoding zlib input blocks costs, on one GPU.

Two runs of word text (16-byte keys, 100-byte values of five 20-byte words
from a small vocabulary, 4 KiB blocks: the workload of tools/lz4_input_probe.py)
stored once per codec, each pair compacted into snappy files with one job in
flight.  Prints one JSON line per job with the block decoder's kernel time
(HIP events, the second of two executions) and GB/s of decoded bytes:

  zlib_dynamic   level 6                      k_decompress_zlib, all stages
  zlib_fixed     Z_FIXED                      no per-block table build
  zlib_huffman   Z_HUFFMAN_ONLY               no matches: tables + symbol walk
  zlib_stored    level 0                      staging and wave copies only
  lz4            liblz4, where installed      k_decompress_lz4
  zstd           the oracle's writer          k_decompress_zstd
  snappy         the oracle's writer          k_decompress

and one line for a single host core running zlib.decompress over the same
level-6 blocks.  The zlib variants leave stages out by their input: stored
has no header work, symbols or matches; huffman has no matches; fixed builds
its tables once per wave.  Only the figures of one run compare: boxes vary
15-25 % run to run.

Usage: python tools/zlib_input_probe.py [entries_per_run] [workdir]
"""
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import oracle  # noqa: E402
import toplingdb_amd as dcw  # noqa: E402
import foreign_lz4 as fl  # noqa: E402
import foreign_zlib as fz  # noqa: E402
from lz4_input_probe import word_entries  # noqa: E402

VARIANTS = (  # name, stored type, encoder or table option, kernel
    ("zlib_dynamic", fz.ZLIB, fz.deflate, "decompress_zlib"),
    ("zlib_fixed", fz.ZLIB, fz.POLICIES["fixed"], "decompress_zlib"),
    ("zlib_huffman", fz.ZLIB, fz.POLICIES["huffman_only"], "decompress_zlib"),
    ("zlib_stored", fz.ZLIB, fz.POLICIES["stored"], "decompress_zlib"),
    ("lz4", fl.LZ4, fl.liblz4_encode, "decompress_lz4"),
    ("zstd", None, 7, "decompress_zstd"),
    ("snappy", None, 1, "decompress"),
)


def write_file(path, entries, btype, enc, streams):
    decoded = [0]

    def codec(raw):
        decoded[0] += len(raw)
        s = enc(raw)
        streams.append((s, len(raw)))
        return btype, fl.frame(s, len(raw))

    if btype is None:
        sst = oracle.build_sst(entries, oracle.default_table_opts(compression=enc))
    else:
        sst = oracle.build_sst(entries, oracle.default_table_opts(compression=0),
                               data_block_codec=codec)
    with open(path, "wb") as f:
        f.write(sst)
    return decoded[0]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="zlp_")
    os.makedirs(work, exist_ok=True)
    runs = [word_entries(n, 1 + r, 1 + r * n) for r in range(2)]
    dcw.init(0)
    lib = dcw.lib()
    lib.dcw_kernel_stats_json.restype = ctypes.c_int32
    lib.dcw_kernel_stats_json.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    decoded_bytes = 0
    for name, btype, enc, kernel in VARIANTS:
        if name == "lz4" and fl.liblz4_encode(b"probe") is None:
            print(json.dumps({"job": name, "skipped": "liblz4.so.1 is not installed"}))
            continue
        streams, paths, dec = [], [], 0
        for r, entries in enumerate(runs):
            paths.append([os.path.join(work, "%s_%d.sst" % (name, r))])
            dec += write_file(paths[-1][0], entries, btype, enc, streams)
        decoded_bytes = dec or decoded_bytes  # the oracle's writers: same blocks
        outd = os.path.join(work, "out_" + name)
        for _ in range(2):
            shutil.rmtree(outd, ignore_errors=True)
            os.makedirs(outd)
            lib.dcw_kernel_stats_reset()
            res = dcw.execute(dcw.make_job(paths, outd, compression=1))
        buf = ctypes.create_string_buffer(16384)
        lib.dcw_kernel_stats_json(buf, 16384)
        k = json.loads(buf.value.decode())[kernel]
        ms = k["ms"] / k["launches"]
        print(json.dumps({"job": name, "kernel": kernel, "in_MB": round(res["in_bytes"] / 1e6, 1),
                          "decoded_MB": round(decoded_bytes / 1e6, 1), "kernel_ms": round(ms, 3),
                          "decoded_GBps": round(decoded_bytes / ms / 1e6, 2)}), flush=True)
        if name == "zlib_dynamic":
            t0 = time.perf_counter()
            for s, _ in streams:
                zlib.decompress(s, -15)
            dt = time.perf_counter() - t0
            print(json.dumps({"job": "host_core_zlib_decompress", "blocks": len(streams),
                              "ms": round(dt * 1e3, 1),
                              "decoded_GBps": round(decoded_bytes / dt / 1e9, 3)}), flush=True)
    dcw.shutdown()
    if len(sys.argv) <= 2:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
