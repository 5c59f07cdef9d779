"""Records the bytes the packs and the GEMM host routes write for the cases of tests/pack_bytes_cases.py, as SHA-256
digests: tests/golden/pack_bytes_parent.json.

The recorded file was written, on the GPU, by the commit BEFORE the pack kernels moved to csrc/conv_pack.hip and their numeric
rules to csrc/pack_terms.h; tests/test_pack_bytes.py holds every later library to it.  Every case runs twice; a case whose
two runs disagree is not recorded: it is listed under "_unstable" and left to the tolerance tests of its route.
"_rerecorded" (written by hand, not by this script) names the digests that were replaced later, and why: a change of
results made on purpose replaces exactly the digests it explains and leaves the others as first recorded.

    python tests/golden/make_pack_bytes_golden.py [OUT]     # rewrite the JSON (only ever from the commit it records)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "pack_bytes_parent.json")


def dump(doc):
    """One case per line."""
    lines = ["{"]
    for i, (k, v) in enumerate(doc.items()):
        lines.append("%s:%s%s" % (json.dumps(k), json.dumps(v, separators=(",", ":")), "," if i + 1 < len(doc) else ""))
    return "\n".join(lines) + "\n}\n"


if __name__ == "__main__":
    import pack_bytes_cases as C
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    doc, unstable = {}, []
    for name in C.CASES:
        a, b = C.run_case(name), C.run_case(name)
        if a != b:
            unstable.append(name)
            print("UNSTABLE %s: %s" % (name, sorted(k for k in a if a[k] != b.get(k))), flush=True)
            continue
        doc[name] = a
    doc["_unstable"] = unstable
    with open(out, "w") as f:
        f.write(dump(doc))
    print("%d cases, %d unstable -> %s (%d bytes)" % (len(doc) - 1, len(unstable), out, os.path.getsize(out)))
