"""The convolution dispatch as a plan (accflow_amd/csrc/conv_plan.cpp), checked without a GPU.

(a) The library's two route queries answer, for the fixed grid of tests/golden/make_conv_route_golden.py and in each of its
    environments, exactly what the library answered before the dispatch became a plan (tests/golden/conv_route_queries.json:
    recorded from the dry-run dispatcher that preceded it).
(b) The plan unit itself, compiled with the host compiler and -fsanitize=address,undefined into a stand-alone driver
    (tests/c_host/conv_plan_driver.cpp; nothing is loaded into Python), over the same grid: the properties listed at
    test_plan_properties.
"""
import importlib.util
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_conv_route_golden", os.path.join(ROOT, "tests", "golden", "make_conv_route_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

ENV_IDS = [G.env_key(e) for e in G.ENVS]
EPI_GRU_ZR = 2


@pytest.fixture(scope="module")
def grid():
    return G.grid()


@pytest.fixture(scope="module")
def golden():
    with open(G.OUT) as f:
        return json.load(f)


_answers = {}


def library_answers(env):
    """The loaded library's answers in a fresh process with this environment (once per module run)."""
    from accflow_amd import build as _b
    _b.build(force=False, verbose=False)
    k = G.env_key(env)
    if k not in _answers:
        _answers[k] = G.query_in_child(env)
    return _answers[k]


def test_grid_is_the_recorded_one(grid, golden):
    assert golden["n"] == len(grid) and golden["grid_sha256"] == G.grid_hash(grid)
    assert sorted(golden["answers"]) == sorted(ENV_IDS)


@pytest.mark.parametrize("env", G.ENVS, ids=ENV_IDS)
def test_route_queries_answer_as_recorded(env, golden):
    got, want = library_answers(env), golden["answers"][G.env_key(env)]
    for key in ("slots", "norm"):
        diff = [i for i, (a, b) in enumerate(zip(got[key], want[key])) if a != b]
        assert len(got[key]) == len(want[key]) and not diff, (key, len(diff), [(i, got[key][i], want[key][i]) for i in diff[:8]])


@pytest.fixture(scope="module")
def driver(tmp_path_factory, grid):
    """(driver executable, file of the grid's descriptors)"""
    import ctypes
    tmp = tmp_path_factory.mktemp("conv_plan")
    exe = str(tmp / "conv_plan_driver")
    csrc = os.path.join(ROOT, "accflow_amd", "csrc")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           os.path.join(csrc, "conv_plan.cpp"), os.path.join(ROOT, "tests", "c_host", "conv_plan_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    path = str(tmp / "descriptors.bin")
    with open(path, "wb") as f:
        for fields in grid:
            f.write(ctypes.string_at(ctypes.byref(G.to_desc(fields)), ctypes.sizeof(G.to_desc(fields))))
    return exe, path


PLAN = ("ok", "family", "tc", "tp", "wc", "wp", "lay", "loop", "tapgemm", "norm", "w4", "mode", "slots", "ch0", "Z")


def run_driver(driver, env):
    exe, path = driver
    e = {k: v for k, v in os.environ.items() if k not in G.SWITCHES}
    e.update(env)
    r = subprocess.run([exe, path], env=e, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])   # (6) the sanitizers report nothing
    rows = []
    for ln in r.stdout.splitlines():
        head, qa, q, s, l, parts = [[int(x) for x in part.split()] for part in ln.split("|")]
        rows.append(dict(valid=head[1], slots=qa[0], norm=qa[1], q=dict(zip(PLAN, q)), s=dict(zip(PLAN, s)), l=dict(zip(PLAN, l)),
                         lok=parts[0], parts=parts[1:]))
    return rows


@pytest.mark.parametrize("env", G.ENVS, ids=ENV_IDS)
def test_plan_properties(env, grid, driver):
    """1. slots and normalise-on-load as planned equal the library's query answers;
    2. planning with want_stats = true and planning the same descriptor with `stats` set and stat_slots = slots give the same
       family, tile, variant and slots, and no tail split (ch0 == 0).  Where the descriptor with `stats` is refused although
       the query reports slots, it is one of the S16 / channel-block forms of the direct kernel (in_fmt, out16, cb), whose
       launches take no statistics - the query never looked at `stats`, before or after the plan - and nothing else;
    3. Z == 1 with statistics, an S16 residual, split_c0, without a workspace, and for an S16 GRU_ZR copy off an octet;
    4. the parts fit the workspace: Z * B * Cout * OH * OW <= kws_elems wherever the workspace is used (Z > 1), for the
       two launches of a tail split as well;
    5. a descriptor the validation rejects yields no plan;
    6. the sanitizers report nothing (run_driver)."""
    rows = run_driver(driver, env)
    lib = library_answers(env)
    assert len(rows) == len(grid)
    assert [r["slots"] for r in rows] == lib["slots"] and [r["norm"] for r in rows] == lib["norm"]          # (1)
    n_stats = n_tail = n_split = 0
    for i, (r, f) in enumerate(zip(rows, grid)):
        q, s, l = r["q"], r["s"], r["l"]
        if not r["valid"]:                                                                                   # (5)
            assert not q["ok"] and not s["ok"] and not l["ok"] and r["slots"] == 0 and r["norm"] == 0, (i, f)
            continue
        assert r["lok"] >= 0, (i, f)
        if q["ok"] and q["slots"] > 0 and f.get("epi", 0) == 0 and f.get("act", 0) == 0 and not f.get("stats"):   # (2)
            if s["ok"]:
                n_stats += 1
                same = ("family", "tc", "tp", "wc", "wp", "lay", "loop", "tapgemm", "norm", "w4", "mode", "slots")
                assert [q[k] for k in same] == [s[k] for k in same] and q["ch0"] == 0 and s["ch0"] == 0 and s["Z"] == 1, (i, f, q, s)
            else:
                assert f.get("in_fmt") or f.get("out16") or f.get("cb"), (i, f, q)
        if l["ok"]:
            nout = f["B"] * f["Cout"] * f["OH"] * f["OW"]
            no_split = (f.get("stats") or f.get("e0_fmt") or f.get("split_c0") or not f.get("kws")
                        or (f.get("out16") and f.get("epi") == EPI_GRU_ZR and (f["Cout"] // 2) % 8))
            if no_split:                                                                                    # (3)
                assert l["Z"] == 1 and r["parts"][0] <= 1 and r["parts"][2] <= 1, (i, f, l, r["parts"])
            if l["ch0"]:
                n_tail += 1
                zh, nh, zt, nt = r["parts"]
                assert nh + nt == nout and (zh == 1 or zh * nh <= f["kws_elems"]) and (zt == 1 or zt * nt <= f["kws_elems"]), (i, f, r)
            else:
                n_split += l["Z"] > 1
                assert l["Z"] == 1 or l["Z"] * nout <= f["kws_elems"], (i, f, l)                             # (4)
        if s["ok"]:
            assert s["Z"] == 1 and s["ch0"] == 0, (i, f, s)                                                  # (3) with statistics
    # the grid reaches what it is meant to reach
    print("with statistics %d, tail splits %d, split-K launches %d" % (n_stats, n_tail, n_split))
    assert min(n_stats, n_tail, n_split) >= 10, (n_stats, n_tail, n_split)
