"""zlib-output probe: what encoding zlib output blocks costs and saves next to
snappy and LZ4, on one GPU.

Two corpora, each run with compression 1 (k_compress), 4 (k_compress_lz4) and
2 (k_compress_zlib) over the same inputs, jobs one at a time, the second of
two executions reported:
  (bench) the benchmark's 8-way workload (bench.py: 8 generated snappy runs,
          16-byte keys, target_file_size 64 MiB, bottommost);
  (words) one run of word text (random words of 3..11 bytes from a vocabulary
          of 700, 1000-byte values) built by the oracle, block_size 4096.
Prints one JSON line per job: the encoder's total time, its microseconds per
uncompressed MB (the kernel statistics keep 1.6 x, 2.6 x resp. 3.6 x the
uncompressed bytes as algorithmic bytes) and the output bytes.  For the zlib
job it then walks the data blocks of the first output file from offset 0 for
as long as they are type-2 blocks (a raw block has no length of its own and
ends the walk) and prints how many of them begin with a fixed and how many
with a dynamic deflate block, and their stored size next to Python's zlib at
level 6, wbits -14, over the same bytes.  Only the figures of one run
compare: boxes vary 15-25 % run to run.

Usage: python tools/zlib_output_probe.py [entries_per_run] [workdir]
"""
import ctypes
import json
import os
import random
import shutil
import sys
import tempfile
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402
import toplingdb_amd as dcw  # noqa: E402

ENCODERS = {1: ("compress", 1.6), 4: ("compress_lz4", 2.6), 2: ("compress_zlib", 3.6)}


def run_job(lib, runs, outd, compression, **kw):
    for _ in range(2):  # the first warms buffers and the page cache
        shutil.rmtree(outd, ignore_errors=True)
        os.makedirs(outd)
        lib.dcw_kernel_stats_reset()
        res = dcw.execute(dcw.make_job(runs, outd, compression=compression,
                                       target_file_size=64 << 20,
                                       bottommost_level=1, **kw))
    buf = ctypes.create_string_buffer(16384)
    lib.dcw_kernel_stats_json(buf, 16384)
    return res, json.loads(buf.value.decode())


def walk_zlib_blocks(path, limit=20000):
    """-> counts over the leading type-2 blocks of the file"""
    data = open(path, "rb").read()
    at, out = 0, dict(blocks=0, fixed=0, dynamic=0, raw_bytes=0, stored=0, zlib6=0)
    while out["blocks"] < limit:
        n = shift = hl = 0
        while at + hl < len(data):
            b = data[at + hl]
            n |= (b & 0x7f) << shift
            shift += 7
            hl += 1
            if not b & 0x80 or hl == 5:
                break
        d = zlib.decompressobj(wbits=-14)
        part = data[at + hl:at + hl + 2 * n + 64]
        try:
            raw = d.decompress(part)
        except zlib.error:
            break
        used = len(part) - len(d.unused_data)
        if not d.eof or len(raw) != n or data[at + hl + used:at + hl + used + 1] != b"\x02":
            break
        out["blocks"] += 1
        out["dynamic" if data[at + hl] >> 1 & 3 == 2 else "fixed"] += 1
        out["raw_bytes"] += n
        out["stored"] += hl + used
        c = zlib.compressobj(6, zlib.DEFLATED, -14)
        out["zlib6"] += hl + len(c.compress(raw) + c.flush())
        at += hl + used + 5
    return out


def word_run(path, entries):
    rng = random.Random(0x70B)
    words = [rng.randbytes(rng.randrange(3, 12)) for _ in range(700)]
    ents = []
    for i in range(entries):
        v = bytearray()
        while len(v) < 1000:
            v += rng.choice(words) + b" "
        ents.append((oracle.make_ikey(b"%016d" % i, 1 + i, 1), bytes(v[:1000])))
    with open(path, "wb") as f:
        f.write(oracle.build_sst(ents, oracle.default_table_opts(block_size=4096)))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 920_000
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="zlo_")
    os.makedirs(work, exist_ok=True)
    dcw.init(0)
    lib = dcw.lib()
    lib.dcw_kernel_stats_json.restype = ctypes.c_int32
    lib.dcw_kernel_stats_json.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    bench_runs = []
    for r in range(8):
        p = os.path.join(work, "in%d.sst" % r)
        dcw.gen_sst(p, seed=0x746F706C696E6721 + r, num_entries=n,
                    seq_base=1 + r * n, compression=1)
        bench_runs.append([p])
    word_run(os.path.join(work, "words.sst"), max(1000, n // 40))
    for corpus, runs, kw in (("bench", bench_runs, {}),
                             ("words", [[os.path.join(work, "words.sst")]],
                              dict(block_size=4096))):
        seen = {}
        for compression, (kernel, factor) in ENCODERS.items():
            outd = os.path.join(work, "out_%s%d" % (corpus, compression))
            res, ks = run_job(lib, runs, outd, compression, **kw)
            k = ks[kernel]
            unc_mb = k["alg_bytes"] / factor / 1e6
            seen[compression] = (1000 * k["ms"] / unc_mb, res["out_bytes"])
            print(json.dumps({
                "corpus": corpus, "compression": compression, "encoder": kernel,
                "launches": k["launches"], "encoder_ms": round(k["ms"], 3),
                "uncompressed_MB": round(unc_mb, 1),
                "us_per_uncompressed_MB": round(seen[compression][0], 2),
                "out_MB": round(res["out_bytes"] / 1e6, 2),
                "work_ms": round(res["work_time_usec"] / 1000.0, 1),
            }), flush=True)
            if compression == 2:
                print(json.dumps(dict(corpus=corpus,
                                      **walk_zlib_blocks(res["files"][0]["path"]))),
                      flush=True)
        print(json.dumps({
            "corpus": corpus,
            "zlib_over_snappy_out_bytes": round(seen[2][1] / seen[1][1], 3),
            "zlib_over_lz4_out_bytes": round(seen[2][1] / seen[4][1], 3),
            "zlib_over_snappy_time_per_MB": round(seen[2][0] / seen[1][0], 2),
            "zlib_over_lz4_time_per_MB": round(seen[2][0] / seen[4][0], 2),
        }), flush=True)
    dcw.shutdown()
    if len(sys.argv) <= 2:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
