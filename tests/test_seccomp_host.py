"""Host side of advise seccomp-profile: getSeccompProfileNextName against the reference's own
table (gadget_test.go's eight cases, recorded in tests/golden/seccomp_nextname.json), Arches,
syscallArrToNameList's sorting and "syscall%d" fallback, the profile builders' JSON and the
MarshalIndent layout collectResult uses.  No GPU."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seccomp_nextname.json")
CASES = json.load(open(GOLDEN))["cases"]


@pytest.fixture(scope="module")
def G(igx):
    return igx.gadgets


def test_golden_has_the_eight_cases():
    assert len(CASES) == 8


@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_next_name_golden(G, case):
    assert G.getSeccompProfileNextName(case["profiles"], case["pod"]) == case["expected"]


def test_next_name_follows_trimleft_and_atoi(G):
    # strings.TrimLeft strips a cutset, not a prefix: "podname-e7" loses its 'e' too
    assert G.getSeccompProfileNextName(["podname-e7"], "podname") == "podname-8"
    # the name itself counts once, and only while the counter is 0; later it trims to "" (no number)
    assert G.getSeccompProfileNextName(["podname-4", "podname"], "podname") == "podname-5"
    assert G.getSeccompProfileNextName(["podname", "podname"], "podname") == "podname-2"
    # Atoi takes a sign; a negative or non-decimal count is never above the counter / is ignored
    assert G.getSeccompProfileNextName(["podname+3"], "podname") == "podname-4"
    assert G.getSeccompProfileNextName(["podname-1_0", "podname- 3", "podname-٣"], "podname") == "podname"
    assert G.getSeccompProfileNextName(["podname-99999999999999999999"], "podname") == "podname"   # out of range


def test_arches(G):
    assert G.Arches() == ["SCMP_ARCH_X86_64", "SCMP_ARCH_X86", "SCMP_ARCH_X32"]
    assert G.Arches("arm64") == ["SCMP_ARCH_ARM", "SCMP_ARCH_AARCH64"]
    assert G.Arches("s390x") == ["SCMP_ARCH_S390", "SCMP_ARCH_S390X"]
    assert G.Arches("mips64") == G.Arches("mips64n32") == ["SCMP_ARCH_MIPS", "SCMP_ARCH_MIPS64", "SCMP_ARCH_MIPS64N32"]
    assert G.Arches("mipsel64") == G.Arches("mipsel64n32")
    assert G.Arches("riscv64") == []
    a = G.Arches()
    a.append("x")
    assert len(G.Arches()) == 3   # a copy each time


def test_name_list_sorting_and_fallback(G):
    v = bytearray(501)
    for i in (0, 1, 3, 59, 157, 317, 499):
        v[i] = 1
    v[500] = 1   # the footer is not a syscall
    names = G.syscallArrToNameList(v)
    assert names == ["close", "execve", "prctl", "read", "seccomp", "syscall499", "write"]
    assert G.syscallArrToNameList(bytes(501)) == []
    # a caller's table; sort.Strings is byte order: capitals first, "syscall10" before "syscall9"
    v = bytearray(501)
    for i in (3, 4, 9, 10):
        v[i] = 1
    assert G.syscallArrToNameList(v, {3: "b", 4: "B"}) == ["B", "b", "syscall10", "syscall9"]
    # a value longer than 500 bytes: only the first 500 are syscalls
    assert G.syscallArrToNameList(bytes(500) + b"\1\1\1") == []


def test_generated_table(igx):
    t = importlib_table(igx)
    assert t[0] == "read" and t[157] == "prctl" and t[317] == "seccomp" and t[59] == "execve"
    assert all(0 <= k < 500 for k in t) and len(set(t.values())) == len(t)


def importlib_table(igx):
    import importlib
    return importlib.import_module(igx.__name__ + "._syscalls").X86_64


def test_linux_seccomp_json(G):
    got = G.go_marshal(G.SyscallNamesToLinuxSeccomp(["close", "read"]), sort_maps=False)
    assert got == ('{"defaultAction":"SCMP_ACT_ERRNO","architectures":["SCMP_ARCH_X86_64","SCMP_ARCH_X86",'
                   '"SCMP_ARCH_X32"],"syscalls":[{"names":["close","read"],"action":"SCMP_ACT_ALLOW"}]}')
    assert json.loads(got)["syscalls"][0].keys() == {"names", "action"}   # empty args: omitempty
    # no architectures on an unknown GOARCH (omitempty); an empty name list stays a list, nil is null
    assert G.go_marshal(G.SyscallNamesToLinuxSeccomp([], "riscv64"), sort_maps=False) == \
        '{"defaultAction":"SCMP_ACT_ERRNO","syscalls":[{"names":[],"action":"SCMP_ACT_ALLOW"}]}'
    assert '"names":null' in G.go_marshal(G.SyscallNamesToLinuxSeccomp(None), sort_maps=False)


def test_seccomp_policy_json(G):
    p = G.syscallNamesToSeccompPolicy(G.SeccompProfileNsName("ns", "pod", False), ["read"], "arm64")
    assert G.go_marshal(p, sort_maps=False) == (
        '{"metadata":{"name":"pod","namespace":"ns","creationTimestamp":null},'
        '"spec":{"defaultAction":"SCMP_ACT_ERRNO","architectures":["SCMP_ARCH_ARM","SCMP_ARCH_AARCH64"],'
        '"syscalls":[{"names":["read"],"action":"SCMP_ACT_ALLOW"}]},"status":{}}')
    p = G.syscallNamesToSeccompPolicy(G.SeccompProfileNsName("ns", "pod", True), ["read"])
    assert p["metadata"] == {"generateName": "pod-", "namespace": "ns", "creationTimestamp": None}
    assert list(p["metadata"]) == ["generateName", "namespace", "creationTimestamp"]


def test_marshal_indent_layout(G):
    out = G.go_marshal({"b": ["x", "y<"], "a": [], "c": None, "B": ["no syscall found"]}, indent="  ")
    assert out == ('{\n  "B": [\n    "no syscall found"\n  ],\n  "a": [],\n  "b": [\n    "x",\n    "y\\u003c"\n  ],\n'
                   '  "c": null\n}')
    assert G.go_marshal({}, indent="  ") == "{}"
