"""The dictionary decoders without a GPU: tools/zstd_dict_host and
tools/lz4_dict_host run the kernels' sources under ASan/UBSan over every
stored block of the GPU test's jobs (tests/foreign_dict.py) and the refusals.
The corpus conditions those jobs rest on are asserted here."""
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import foreign_dict as fd  # noqa: E402
import foreign_lz4 as fl  # noqa: E402
import foreign_zstd as fz  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_tool(d, name, sections):
    exe = str(d / name)
    r = subprocess.run(
        ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I", os.path.join(REPO, "toplingdb_amd", "csrc"), "-o", exe,
         os.path.join(REPO, "tools", name, name + ".cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(d / "corpus.bin", "wb") as f:
        for dic, blocks in sections:
            f.write(struct.pack("<III", len(dic), 0xfffffffe, 0) + dic)
            for payload, raw in blocks:
                f.write(struct.pack("<III", len(payload), len(raw or b""),
                                    0xffffffff if raw is None else len(raw)) +
                        payload + (raw or b""))
    return subprocess.run([exe, str(d / "corpus.bin")], capture_output=True, text=True,
                          timeout=300)


def test_corpus_conditions():
    for cap in (4096, 16384):
        assert fd.trained(cap)[:4] == b"\x37\xa4\x30\xec" and len(fd.trained(cap)) == cap
    assert fd.trained(4096)[6:8] != b"\0\0"  # a 4-byte Dictionary_ID field
    for name, treeless in (("trained_4k", True), ("trained_1k", False)):
        infos = [fd.frame_info(fl.unframe(p)[1]) for p, _ in fd.zstd_job(name)[0][3]]
        dic = fd.zstd_job(name)[0][4]
        assert all(i[0] == int.from_bytes(dic[4:8], "little") for i in infos)
        assert any(i[1] == 3 for i in infos) == treeless
    assert not fd.zstd_job("raw_content")[0][4].startswith(b"\x37\xa4\x30\xec")
    assert all(r[3] is None for r in fd.refusals().values())  # libzstd refuses each


@pytest.mark.parametrize("kind", ["zstd", "lz4"])
def test_tool(tmp_path, kind):
    jobs = ([fd.zstd_job(n)[0] for n in fd.ZSTD_CASES] if kind == "zstd" else
            [fd.lz4_job(n)[0] for n in sorted(fd.LZ4_CASES)])
    bad = [(d, [(payload, None)]) for d, t, payload, _ in fd.refusals().values()
           if (t == fz.ZSTD) == (kind == "zstd")]
    r = run_tool(tmp_path, kind + "_dict_host", [(j[4], j[3]) for j in jobs] + bad)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.split("\n")[-3]
    n = sum(len(j[3]) for j in jobs)
    head = ("%d dictionaries (1 refused), %d records (%d decoded, %d malformed," % (
        len(jobs) + len(bad), n + len(bad), n, len(bad)) if kind == "zstd" else
        "%d dictionaries, %d records (%d malformed," % (
            len(jobs) + len(bad), n + len(bad), len(bad)))
    assert last.startswith(kind + "_dict_host: " + head), last
    assert " 0 small" not in last and " 0 large" not in last and " 0 on the LDS" not in last
