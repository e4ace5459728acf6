"""Child process of tests/test_foreign_input_gpu.py's decoder-variant tests.

DCW_DEC_PIPE / DCW_DECOMP_V are read once per process, so each variant runs
in a fresh interpreter started by the parent with the variable set.  This
script only executes the jobs of a manifest on the GPU worker and records
what it wrote; the parent compares the outputs with the oracle's.

  python foreign_variant_runner.py <manifest.json>

manifest: {"result": path, "jobs": [{"name", "runs", "out_dir", "kw"}]}
result:   {name: {"files": [{"path", "file_number"}], "out_entries"}
                 | {"error": text}}
The first job that fails ends the run (nothing more is started on the GPU).
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(manifest_path):
    sys.path.insert(0, REPO)
    import toplingdb_amd as dcw

    with open(manifest_path) as f:
        man = json.load(f)
    results = {}
    dcw.init(0)
    for job in man["jobs"]:
        os.makedirs(job["out_dir"])
        try:
            res = dcw.execute(
                dcw.make_job(job["runs"], job["out_dir"], **job["kw"]))
        except RuntimeError as e:
            results[job["name"]] = {"error": str(e)}
            break
        results[job["name"]] = {
            "out_entries": res["out_entries"],
            "files": [{"path": f["path"], "file_number": f["file_number"]}
                      for f in res["files"]],
        }
    with open(man["result"], "w") as f:
        json.dump(results, f)
    dcw.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
