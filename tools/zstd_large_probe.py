"""Large-frame zstd input probe: k_decompress_zstd_large against the host leg.

For each block size (16 KiB and 64 KiB) one bottommost job of two runs of
zstd files (`oracle.build_sst(compression=7)`), about 64 MB stored each with
the default entry count; entries of word + number + 48 random bytes + a
repeated word, no output compression.  Every data block is a frame beyond the
small decoder's staging size.  After a warm-up of each leg the GPU path and
DCW_ZSTD_LARGE_HOST=1 alternate in one process, `reps` times each; wall time
around `dcw.execute`.  Prints one JSON line per block size: sorted times,
medians and spread (max - min over median) of both legs, and the statistics
entry of `decompress_zstd_large` from the last GPU-leg job.

Usage: python tools/zstd_large_probe.py [entries_per_run] [reps] [workdir]
"""
import ctypes
import json
import os
import random
import shutil
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import oracle  # noqa: E402
import toplingdb_amd as dcw  # noqa: E402


def entries(n, seed, seq_base):
    rng = random.Random(seed)
    words = [b"alpha", b"bravo", b"charlie", b"delta", b"echo", b"foxtrot"]
    keys = sorted(rng.sample(range(10 ** 15), n))
    return [(oracle.make_ikey(b"%016d" % k, seq_base + i, 1),
             b"%s-%09d-%s-%s" % (w, rng.randrange(10 ** 9), rng.randbytes(48), w * 3))
            for i, k in enumerate(keys) for w in (rng.choice(words),)]


def execute_ms(runs, outd, host_leg):
    shutil.rmtree(outd, ignore_errors=True)
    os.makedirs(outd)
    if host_leg:
        os.environ["DCW_ZSTD_LARGE_HOST"] = "1"
    else:
        os.environ.pop("DCW_ZSTD_LARGE_HOST", None)
    t0 = time.perf_counter()
    res = dcw.execute(dcw.make_job(runs, outd, compression=0, bottommost_level=1))
    return (time.perf_counter() - t0) * 1e3, res


def summary(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_sorted": [round(x, 1) for x in ms], "median_ms": round(med, 1),
            "spread_pct": round(100 * (ms[-1] - ms[0]) / med, 1)}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 870_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="zlp_")
    os.makedirs(work, exist_ok=True)
    ents = [entries(n, 1 + r, 1 + r * n) for r in range(2)]
    dcw.init(0)
    lib = dcw.lib()
    lib.dcw_kernel_stats_json.restype = ctypes.c_int32
    lib.dcw_kernel_stats_json.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    for bs in (16384, 65536):
        runs = []
        for r, e in enumerate(ents):
            p = os.path.join(work, "bs%d_run%d.sst" % (bs, r))
            with open(p, "wb") as f:
                f.write(oracle.build_sst(e, oracle.default_table_opts(
                    compression=7, block_size=bs)))
            runs.append([p])
        outd = os.path.join(work, "out")
        ms = {False: [], True: []}
        for rep in range(reps + 1):  # rep 0 warms both legs up
            for host_leg in (False, True):
                if not host_leg:
                    lib.dcw_kernel_stats_reset()
                t, res = execute_ms(runs, outd, host_leg)
                if not host_leg:
                    buf = ctypes.create_string_buffer(16384)
                    lib.dcw_kernel_stats_json(buf, 16384)
                    kstat = json.loads(buf.value.decode())["decompress_zstd_large"]
                if rep:
                    ms[host_leg].append(t)
        print(json.dumps({
            "block_size": bs, "in_MB": round(res["in_bytes"] / 1e6, 1),
            "in_entries": res["in_entries"], "out_entries": res["out_entries"],
            "gpu": summary(ms[False]), "host": summary(ms[True]),
            "decompress_zstd_large": kstat}), flush=True)
    dcw.shutdown()
    if len(sys.argv) <= 3:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
