"""The dispatch plan's fingerprint against recorded values (no GPU needed).

tests/golden/plan_stats.json holds gpfit.plan_check's 11 stats for every environment of
test_plan.ENVS over a grid of block-column and particle counts, recorded before the planner moved
into csrc/gpf_plan.hip (plan_factor): a change of the host-side planning code that is meant to leave
every launch as it was must reproduce them exactly. A deliberate schedule change regenerates the
file (python tests/test_plan_golden.py --regen, with the library built) and says so.
"""
import json
import os
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "plan_stats.json"
if __name__ == "__main__":  # (under pytest, conftest.py puts the package on the path)
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "gaussian-process_amd"))
NT = [1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 64, 128]
PC = [1, 2, 7, 8, 16, 17, 32, 33, 64]
KEYS = ["launches", "workgroups", "whole_tiles", "split_tiles", "S", "Smax", "groups", "diag_workgroups",
        "syrk_workgroups", "persistent", "lead_launches"]
# a particle group one short of / just past the 12 bits gpf::lall_tag carries the group size in
GC_ENV = {"GPF_EARLY_DIAG": "1", "GPF_PERSIST": "0"}
GC_NT = 4


def _environment(kv):
    """test_plan's env fixture: the launch-plan knobs apply to the per-block-column launches."""
    e = dict(kv)
    if kv and "GPF_PERSIST" not in kv:
        e["GPF_PERSIST"] = "0"
    return e


def _apply(kv, setenv, delenv):
    for k in [k for k in os.environ if k.startswith("GPF_")]:
        delenv(k)
    for k, v in _environment(kv).items():
        setenv(k, v)


def _grid(plan_check):
    return [[plan_check(pc, nt)[k] for k in KEYS] for nt in NT for pc in PC]


def _load():
    with open(GOLDEN) as f:
        return json.load(f)


def _envs():
    from test_plan import ENVS
    return ENVS


@pytest.mark.parametrize("i", range(len(_envs())),
                         ids=lambda i: ",".join(f"{k}={v}" for k, v in _envs()[i].items()) or "default")
def test_plan_stats_match_the_recorded_ones(monkeypatch, i):
    import gpfit
    gold = _load()
    assert (gold["nt"], gold["pc"], gold["keys"]) == (NT, PC, KEYS)
    assert [g["env"] for g in gold["envs"]] == _envs(), "regenerate the golden file: test_plan.ENVS changed"
    _apply(_envs()[i], monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    got = _grid(gpfit.plan_check)
    want = gold["envs"][i]["stats"]
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"nt={NT[j // len(PC)]} pc={PC[j % len(PC)]}: {dict(zip(KEYS, g))} != {dict(zip(KEYS, w))}"
    assert len(got) == len(want)


def test_group_size_past_the_piece_tag(monkeypatch):
    """4095 particles in one group still fit the look-ahead pieces' tag and plan as recorded; 4096 do
    not: their plan must pass the check and be the plan without the pieces (GPF_LA_ALL=0)."""
    import gpfit
    gold = _load()["gc_bound"]
    assert gold["env"] == GC_ENV and gold["nt"] == GC_NT
    _apply(GC_ENV, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    st = gpfit.plan_check(4095, GC_NT)
    assert [st[k] for k in KEYS] == gold["4095"]
    big = gpfit.plan_check(4096, GC_NT)
    monkeypatch.setenv("GPF_LA_ALL", "0")
    assert st["workgroups"] > gpfit.plan_check(4095, GC_NT)["workgroups"]  # (4095: the pieces are on)
    assert big == gpfit.plan_check(4096, GC_NT)
    assert big["diag_workgroups"] == 4096 * GC_NT and big["groups"] == 1


if __name__ == "__main__":
    if "--regen" not in sys.argv:
        sys.exit("usage: python tests/test_plan_golden.py --regen  (rewrites tests/golden/plan_stats.json)")
    import gpfit

    def setenv(k, v):
        os.environ[k] = v

    out = {"nt": NT, "pc": PC, "keys": KEYS, "envs": []}
    for kv in _envs():
        _apply(kv, setenv, os.environ.pop)
        out["envs"].append({"env": kv, "stats": _grid(gpfit.plan_check)})
    _apply(GC_ENV, setenv, os.environ.pop)
    st = gpfit.plan_check(4095, GC_NT)
    out["gc_bound"] = {"env": GC_ENV, "nt": GC_NT, "4095": [st[k] for k in KEYS]}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {GOLDEN}")
