"""Hand cases for the host restatements of profile cpu (tests/stack_ref.py), which the device
tests compare with: the dict interner, findKernelSymbol (tracer.go:184-208) with its quirks,
readKernelSymbols, and the probe + collectResult.  No GPU."""
import json

import pytest

from stack_ref import (KSYM_HAND_CASES, NO_COL, DictInterner, ProfileCpuRef, find_kernel_symbol,
                       read_kernel_symbols)


def test_dict_interner_ids_by_first_appearance():
    t = DictInterner()
    assert t.add([b"a" * 8, b"b" * 8, b"a" * 8]) == [0, 1, 0]
    # an invalid first occurrence interns nothing; the valid one after it gets the next id
    assert t.add([b"c" * 8, b"c" * 8, b"b" * 8, b"d" * 8], [0, 1, 1, 1]) == [NO_COL, 2, 1, 3]
    assert t.rows == [b"a" * 8, b"b" * 8, b"c" * 8, b"d" * 8]
    whole, split = DictInterner(), DictInterner()
    stream = [bytes([x % 7]) * 8 for x in (3, 1, 3, 9, 2, 1, 12, 5)]
    assert whole.add(stream) == split.add(stream[:3]) + split.add(stream[3:4]) + split.add(stream[4:])


@pytest.mark.parametrize("addrs,ip,want", KSYM_HAND_CASES)
def test_find_kernel_symbol_hand_cases(addrs, ip, want):
    assert find_kernel_symbol(addrs, ip) == want


def test_read_kernel_symbols():
    text = ("ffffffff81000000 T _text\n"
            "ffffffff81000040 t secondary_startup_64\n"
            "short line\n"
            "\n"
            "ffffffffc0001000 t acpi_video_unregister_backlight      [video]\n")
    assert read_kernel_symbols(text) == [(0xffffffff81000000, "_text"), (0xffffffff81000040, "secondary_startup_64"),
                                         (0xffffffffc0001000, "acpi_video_unregister_backlight")]
    for bad in ("zzzz T x\n", "0x10 T x\n", "+10 T x\n", "1_0 T x\n", "10000000000000000 T x\n"):
        with pytest.raises(ValueError):
            read_kernel_symbols(bad)


KA = 0xffffffff81000000
SYMS = [(KA, "a"), (KA + 0x100, "b"), (KA + 0x200, "c")]


def _stack(*frames, depth=4):
    return b"".join(f.to_bytes(8, "little") for f in frames + (0,) * (depth - len(frames)))


def _feed(ref, samples):
    cols = list(zip(*samples))
    ref.feed(*[list(c) for c in cols])


def test_profile_cpu_probe_and_collect():
    comm = b"bash".ljust(16, b"\0")
    k1, k2, u1 = _stack(KA + 0x110, KA + 4), _stack(KA + 0x210), _stack(0x400000, 0x400100, 0x400200)
    #            pid tid mntns comm  ip           kstack ks  ustack us
    samples = [(7, 7, 99, comm, KA + 0x110, k1, 0, u1, 0),
               (7, 0, 99, comm, KA + 0x110, k1, 0, u1, 0),          # tid 0: dropped, interns nothing
               (7, 8, 99, comm, 0x400000, k2, 0, u1, 0),            # user ip: kernel_ip stays 0
               (7, 7, 99, comm, KA + 0x110, k1, 0, u1, 0),
               (9, 9, 98, comm, KA + 0x110, k1, -14, u1, -17)]      # both walks failed: the errors are the ids
    ref = ProfileCpuRef(kallsyms=SYMS)
    _feed(ref, samples[:2])
    _feed(ref, samples[2:])
    assert list(ref.counts.items()) == [((KA + 0x110, 99, 7, 1, 0, comm), 2), ((0, 99, 7, 1, 2, comm), 1),
                                        ((0, 98, 9, -17, -14, comm), 1)]
    rep = ref.reports()
    # ascending count, ties in first-occurrence order
    assert [(r["Pid"], r["Count"]) for r in rep] == [(7, 1), (9, 1), (7, 2)]
    assert rep[0]["KernelStack"] == ["c"] and rep[0]["UserStack"] == ["[unknown]"] * 3
    assert rep[1]["KernelStack"] == [] and rep[1]["UserStack"] == []
    assert rep[2]["KernelStack"] == ["b", "a"]
    assert json.loads(ref.stop())[1] == {"comm": "bash", "pid": 9, "count": 1}

    idle = ProfileCpuRef(include_idle=True, user_stack_only=True, kallsyms=SYMS)
    _feed(idle, samples)
    # no kernel stack: kern_stack_id -1, kernel_ip 0 for every sample; the idle sample counts
    assert list(idle.counts.items()) == [((0, 99, 7, 0, -1, comm), 4), ((0, 98, 9, -17, -1, comm), 1)]
    konly = ProfileCpuRef(kernel_stack_only=True, kallsyms=SYMS)
    _feed(konly, samples)
    assert list(konly.counts.items()) == [((KA + 0x110, 99, 7, -1, 0, comm), 2), ((0, 99, 7, -1, 1, comm), 1),
                                          ((0, 98, 9, -1, -14, comm), 1)]
