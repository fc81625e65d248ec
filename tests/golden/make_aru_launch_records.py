"""Records tests/golden/aru_launch_records.json: what the ARU engine launches, and what it books for each launch, for the cases of
tests/launch_records.py.  The file is an expectation for refactors of the launchers, so it is recorded on the PARENT of the commit that changes
them (its built tree, with this script and tests/launch_records.py copied in), on the GPU, and never on the branch under test.

Run:  python tests/golden/make_aru_launch_records.py <hash of the recorded commit> [output file]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import launch_records as lr  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "aru_launch_records.json")
    doc = {"recorded_on_commit": commit, "pages": lr.PAGES, "cases": {}}
    for name, kw, env in lr.CASES:
        doc["cases"][name] = {"config": kw, "env": env, "records": lr.records(kw, env)}
        print(name, len(doc["cases"][name]["records"]), "records", flush=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0)
    print("wrote", out)


if __name__ == "__main__":
    main()
