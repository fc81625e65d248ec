"""Same launches, same accounting: the ARU engine's launch records of one batch call against records taken on the commit BEFORE the launchers
were put on one chunk walker (csrc/launch_plan.h, for_chunks in csrc/aru_engine.hip).

tests/golden/aru_launch_records.json was recorded by tests/golden/make_aru_launch_records.py on the commit it names, not on the code under test.
Each case (tests/launch_records.py) loads a model with seeded weights in a fresh handle, its environment set before the load, and runs ONE batch
call of five pages in asep_aru_profile mode 2: with attention that is 15 problems, more than the MAXP = 12 of one launch, so the second chunk of
every split launch is compared too.  Kernel names (with their layer texts) and call counts must be equal, in the report's order; flops, bytes and
executed flops must be equal as printed (%.6e).  With the kernels' argument structs unchanged, that holds a refactor of the launchers to the
kernels, grids and sums of before."""
import json
import os

import pytest

import launch_records as lr

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aru_launch_records.json")) as f:
    GOLDEN = json.load(f)


def test_the_golden_names_its_commit_and_covers_the_cases():
    assert len(GOLDEN["recorded_on_commit"]) == 40
    assert [tuple(p) for p in GOLDEN["pages"]] == lr.PAGES
    assert list(GOLDEN["cases"]) == [name for name, _, _ in lr.CASES]
    for name, kw, env in lr.CASES:
        assert GOLDEN["cases"][name]["config"] == kw and GOLDEN["cases"][name]["env"] == env, name


@pytest.mark.parametrize("name,kw,env", lr.CASES, ids=[c[0] for c in lr.CASES])
def test_launch_records_equal_the_parent_commits(name, kw, env, monkeypatch):
    got = lr.records(kw, env, setenv=monkeypatch.setenv, delenv=lambda k: monkeypatch.delenv(k, raising=False))
    want = GOLDEN["cases"][name]["records"]
    assert [r[0] for r in got] == [r[0] for r in want], name                     # kernels with their layer texts, in launch order
    for g, w in zip(got, want):
        assert g == w, f"{name}: {g[0]}: calls / flops / bytes / executed flops {g[1:]} against {w[1:]}"
    if kw.get("graph", "ARU") == "ARU":                                           # 15 problems: the split launches' second chunk is in the records
        assert any("+..(12)" in r[0] for r in got) and len(lr.PAGES) * 3 > 12
