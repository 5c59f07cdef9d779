"""Records what accflow_amd.ops hands to the kernel library for the cases of tests/conv_desc_cases.py:
tests/golden/conv_desc_parent.json.

The recorded file was written, on the GPU, by the commit BEFORE the four hand-written descriptor fills of ops.py became one
builder (ops._conv_desc); tests/test_conv_desc.py holds every later ops.py to it, call by call and field by field.  See
tests/conv_desc_cases.py for what a record holds and how pointers are labelled.

    python tests/golden/make_conv_desc_golden.py [OUT]     # rewrite the JSON (only ever from the commit it records)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "conv_desc_parent.json")


def dump(doc):
    """One case per line."""
    lines = ["{"]
    for i, (k, v) in enumerate(doc.items()):
        lines.append("%s:%s%s" % (json.dumps(k), json.dumps(v, separators=(",", ":")), "," if i + 1 < len(doc) else ""))
    return "\n".join(lines) + "\n}\n"


if __name__ == "__main__":
    import conv_desc_cases as C
    from accflow_amd import ops
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    doc = {}
    for name in C.CASES:
        rec = C.run_case(ops, name)
        doc[name] = {k: v for k, v in rec.items() if not k.startswith("_")}
        assert not rec["guard_tripped"], name
    with open(out, "w") as f:
        f.write(dump(doc))
    print("%d cases -> %s (%d bytes)" % (len(doc), out, os.path.getsize(out)))
