"""The host parsers of libigx under AddressSanitizer + UndefinedBehaviorSanitizer (a separate
host build, tests/sanitize/Makefile): igx_filter_parse over every filter_test.go row
(tests/golden/filter_table.json), igx_regex_compile_blob over the regex tests' patterns,
igx_sort_prepare over sort_test.go-style sortBy lists, then seeded random patterns and filter
strings.  The kernels' scalar predicate core (csrc/k_pred.h) runs there too, on the host, over
the value pools of pred_reference.py with match_value's bit as the expected one; the driver
stops at the first mismatch.  Any sanitizer report fails the run (-fno-sanitize-recover, non-zero exit)."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = os.path.join(HERE, "sanitize")


def _pred_lines():
    """P lines: kind, width, cmp, negate, value, reference (zero-extended hex u64), IN count, and
    the bit pred_reference.match_value expects."""
    import pred_reference as R
    kinds = {"int": 0, "uint": 1, "float": 2}   # IGX_KIND_*

    def raw(col, p):   # a value as the column holds it / a reference as igx_pred.ref holds it
        return int.from_bytes(R.ref_bytes(col, p), "little")

    def line(col, v, p, cnt=0):
        return (f"P\t{kinds[col.kind]} {col.width} {p.op} {int(p.negate)} {raw(col, R.Pred(0, R.EQ, v)):x} "
                f"{raw(col, p):x} {cnt} {int(R.match_value(col, v, p))}")

    out = []
    for kind in ("int", "uint"):
        for width in (1, 2, 4, 8):
            col, refs = R.Column(kind, width, []), R.int_pool(kind, width)
            for ref in refs:
                for v in R.int_values(kind, width, refs):
                    out += [line(col, v, R.Pred(0, op, ref, neg)) for op in R.OPS for neg in (False, True)]
    for width in (4, 8):
        col = R.Column("float", width, [])
        for ref in R.FLOAT_REFS:
            for v in R.float_values(width):
                out += [line(col, v, R.Pred(0, op, ref, neg)) for op in R.OPS for neg in (False, True)]
    for kind in ("int", "uint"):
        for width in (1, 2, 4, 8):
            col, pool = R.Column(kind, width, []), R.int_pool(kind, width)
            for cnt in sorted(c for c in {1, 2, 8 // width} if c <= 8 // width):
                for k in range(len(pool)):   # sets of cnt members starting at every pool entry
                    members = [pool[(k + 3 * i) % len(pool)] for i in range(cnt)]
                    for v in R.int_values(kind, width, members):
                        out += [line(col, v, R.Pred(0, R.IN, members, neg), cnt) for neg in (False, True)]
    return out


def _corpus(path):
    g = json.load(open(os.path.join(HERE, "golden", "filter_table.json")))
    from test_regex_host import ASSERT_PATTERNS, FOLD_PATTERNS, PATTERNS
    lines = [f"F\t{r['filter']}" for r in g["rows"]]
    lines += [f"R\t{p}" for p in PATTERNS + ASSERT_PATTERNS + FOLD_PATTERNS]
    lines += ["R\t\\p{Greek}", "R\t[[:alpha:][:^digit:]]{2,5}", "R\t\\Qa.b\\E\\101", "R\t(?m)^$|\\b\\B"]
    lines += ["S\tint,-uint8,nope,virt,ext", "S\t,-,--int", "S\tstring,-string,float64,bool"]
    lines += _pred_lines()
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(x.replace("\n", " ") for x in lines) + "\n")


@pytest.mark.timeout(600)
def test_host_parsers_under_asan_ubsan(tmp_path):
    b = subprocess.run(["make", "-s", "-C", SAN], capture_output=True, text=True, timeout=540)
    assert b.returncode == 0, b.stderr[-3000:]
    corpus = str(tmp_path / "corpus.txt")
    _corpus(corpus)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(SAN, "build", "san_main"), corpus], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "SAN_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
