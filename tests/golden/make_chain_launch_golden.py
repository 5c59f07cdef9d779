"""Records what every schedule of AccFlow's fusion chain hands to the kernel library, for the cases of
tests/test_chain_launches.py: tests/golden/chain_launches_parent.json.

The recorded file was written, on the GPU, by the commit BEFORE the copies of the fusion step, the chain loop, the warm loop and
the side-stream harness in accflow_amd/networks/AccFlow_.py and accflow_amd/parallel.py became one each; its "recorded_at" names
that commit.  tests/test_chain_launches.py holds every later tree to it, call by call.

    python tests/golden/make_chain_launch_golden.py COMMIT [OUT]     # rewrite the JSON (only ever in a tree of COMMIT)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "chain_launches_parent.json")


def dump(doc):
    """One distinct call and one case per line."""
    def rows(items):
        return ",\n".join(json.dumps(v, separators=(",", ":")) for v in items)
    cases = ",\n".join("%s:%s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in doc["cases"].items())
    return '{"recorded_at":%s,\n"distinct":[\n%s\n],\n"cases":{\n%s\n}}\n' % (json.dumps(doc["recorded_at"]), rows(doc["distinct"]), cases)


if __name__ == "__main__":
    import test_chain_launches as T
    from accflow_amd import ops
    commit = sys.argv[1]
    assert len(commit) == 40, "the full hash of the commit this tree is"
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    table, cases = {}, {}
    for name in T.CASES:
        calls, returns, tripped, _ = T.run_case(ops, name)
        assert not tripped, name
        cases[name] = {"returns": returns, "calls": [table.setdefault(c, len(table)) for c in calls]}
        print("%-40s %5d calls, %4d distinct so far" % (name, len(calls), len(table)))
    with open(out, "w") as f:
        f.write(dump({"recorded_at": commit, "distinct": [list(c) for c in table], "cases": cases}))
    assert json.load(open(out))["cases"].keys() == cases.keys()
    print("%d cases -> %s (%d bytes)" % (len(cases), out, os.path.getsize(out)))
