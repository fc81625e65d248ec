"""Records tests/golden/split_walk_down_golden.json: digests (float64 sums as hex, CRC-32) of what the f32s level-0 DOWN walker computes for the
cases of tests/split_walk_down_cases.py: the block's output and the level-1 block's output, which is a function of the DOWN block's pool alone.
The file is an expectation for changes of res8ws_kernel<false> that must not move a bit, so it is recorded on the PARENT of the commit that
changes the kernel (its built tree, with this script and tests/split_walk_down_cases.py copied in), on the GPU, and never on the branch under
test.

Run:  python tests/golden/make_split_walk_down_golden.py <hash of the recorded commit> [output file]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import split_walk_down_cases as sc  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "split_walk_down_golden.json")
    doc = {"recorded_on_commit": commit, "cases": {}}
    for name, pages, kind, mvn in sc.CASES:
        res = sc.run(pages, kind, mvn, "1")
        doc["cases"][name] = {"pages": pages, "image": kind, "mvn": mvn,
                              "digests": {n: [sc.digest(a) for a in res[n]] for n in (sc.D0, sc.D1)}}
        print(name, flush=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=0)
    print("wrote", out)


if __name__ == "__main__":
    main()
