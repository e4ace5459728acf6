"""LZ4-input probe: what decoding LZ4 input blocks costs, on one GPU.

  (a) two runs whose data blocks are LZ4 (type 4)       -> snappy files
  (b) the same entries in snappy files (the twins)       -> snappy files

16-byte keys, 100-byte values of five 20-byte words from a small vocabulary
(both codecs compress them), 4 KiB blocks, so every block takes the LDS
decoders.  The LZ4 streams come from liblz4 (LZ4_compress_default), which
must be installed.  Jobs run one at a time; the second of two executions is reported.  Prints one JSON line per
job: ms_decode, the decode-side kernel times, and for the block decoder of
each job (decompress_lz4 / decompress) ms per launch and us per decoded MB.
Only the two figures of one run compare: boxes vary 15-25 % run to run.

Usage: python tools/lz4_input_probe.py [entries_per_run] [workdir]
"""
import ctypes
import json
import os
import random
import shutil
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import oracle  # noqa: E402
import toplingdb_amd as dcw  # noqa: E402
import foreign_lz4 as fl  # noqa: E402

DECODE_KERNELS = ("verify_checksum", "decompress", "decompress_lz4",
                  "count_entries", "decode_entries")


def word_entries(n, seed, seq_base):
    rng = random.Random(99)
    words = [rng.randbytes(20) for _ in range(512)]
    rng = random.Random(seed)
    keys = sorted(rng.sample(range(10 ** 15), n))
    return [(oracle.make_ikey(b"%016d" % k, seq_base + i, 1),
             b"".join(rng.choices(words, k=5))) for i, k in enumerate(keys)]


def write_pair(work, name, entries):
    """-> (LZ4 file, snappy twin, decoded MB of the data blocks)"""
    if fl.liblz4_encode(b"probe") is None:
        sys.exit("liblz4.so.1 is not installed: no encoder for this probe")
    enc = fl.liblz4_encode
    decoded = [0]

    def codec(raw):
        decoded[0] += len(raw)
        return fl.LZ4, fl.frame(enc(raw), len(raw))

    paths = []
    for tag, kw in (("lz4", dict(data_block_codec=codec)), ("snappy", {})):
        to = oracle.default_table_opts(compression=0 if kw else 1)
        paths.append(os.path.join(work, "%s_%s.sst" % (name, tag)))
        with open(paths[-1], "wb") as f:
            f.write(oracle.build_sst(entries, to, **kw))
    return paths[0], paths[1], decoded[0] / 1e6


def run_job(lib, runs, outd):
    for attempt in range(2):
        shutil.rmtree(outd, ignore_errors=True)
        os.makedirs(outd)
        lib.dcw_kernel_stats_reset()
        res = dcw.execute(dcw.make_job(runs, outd, compression=1))
    buf = ctypes.create_string_buffer(16384)
    lib.dcw_kernel_stats_json(buf, 16384)
    return res, json.loads(buf.value.decode())


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="l4p_")
    os.makedirs(work, exist_ok=True)
    pairs = [write_pair(work, "run%d" % r, word_entries(n, 1 + r, 1 + r * n))
             for r in range(2)]
    decoded_mb = sum(p[2] for p in pairs)
    dcw.init(0)
    lib = dcw.lib()
    lib.dcw_kernel_stats_json.restype = ctypes.c_int32
    lib.dcw_kernel_stats_json.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    for tag, col, kernel in (("a_lz4_inputs", 0, "decompress_lz4"),
                             ("b_snappy_twins", 1, "decompress")):
        res, ks = run_job(lib, [[p[col]] for p in pairs],
                          os.path.join(work, "out_" + tag[0]))
        k = ks[kernel]
        print(json.dumps({
            "job": tag,
            "in_MB": round(res["in_bytes"] / 1e6, 1),
            "decoded_MB": round(decoded_mb, 1),
            "in_entries": res["in_entries"],
            "kernels_ms": {x: round(ks[x]["ms"], 3) for x in DECODE_KERNELS
                           if x in ks},
            kernel + "_ms_per_launch": round(k["ms"] / k["launches"], 3),
            kernel + "_us_per_decoded_MB":
                round(1000 * k["ms"] / k["launches"] / decoded_mb, 2),
            "work_ms": round(res["work_time_usec"] / 1000.0, 1),
        }), flush=True)
    dcw.shutdown()
    if len(sys.argv) <= 2:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
