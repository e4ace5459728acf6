"""Decode rate of the dictionary kernels next to the plain ones.

The same record text as zstd input blocks coded with and without a trained
dictionary, at block sizes 4096 (k_decompress_zstd[_dict]) and 16384
(k_decompress_zstd_large[_dict]); each leg is one bottommost job run four
times.  Prints the stored + decoded bytes of one launch per leg; the kernel
times come from running it, from the repository root, as
  rocprofv3 --kernel-trace --stats -d OUT -- python3 tools/dict_rate_probe.py [entries]
"""
import os
import random
import sys
import tempfile

sys.path[:0] = [".", "tests"]
import oracle  # noqa: E402
import toplingdb_amd as dcw  # noqa: E402
import foreign_corpus as fc  # noqa: E402
import foreign_dict as fd  # noqa: E402
import foreign_lz4 as fl  # noqa: E402
import foreign_zstd as fz  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 40000
rng = random.Random(5)
kvs = [(fc.ukey(i), 1 + i, fc.TYPE_VALUE, fz._record_text(480, rng)) for i in range(N)]
dcw.init(0)
tmp = tempfile.mkdtemp(dir="/dev/shm")
for bs, cap in ((4096, 4096), (16384, 16384)):
    dic = fd.trained(cap)
    for leg in ("dict", "plain"):
        nbytes = [0]

        def choose(i, raw):
            f = fd.compress(raw, dic, 1) if leg == "dict" else fz.compress(raw, 1)
            nbytes[0] += len(fz.frame_block(f, len(raw))) + len(raw)
            return fz.ZSTD, f

        _, sst, _, _ = fl.build_pair(kvs, choose, block_size=bs)
        if leg == "dict":
            sst = fd.add_dict_block(sst, dic)
        p = os.path.join(tmp, "in_%d_%s.sst" % (bs, leg))
        with open(p, "wb") as fh:
            fh.write(sst)
        for rep in range(4):
            out = os.path.join(tmp, "out_%d_%s_%d" % (bs, leg, rep))
            os.makedirs(out)
            r = dcw.execute(dcw.make_job([[p]], out, compression=0, bottommost_level=1))
            assert r["out_entries"] == N
        print("LEG bs=%d %s bytes_per_launch=%d launches=4" % (bs, leg, nbytes[0]), flush=True)
dcw.shutdown()
