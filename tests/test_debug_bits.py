"""The AZTOT_DEBUG switches have one list of names in C++ (`enum DebugBit`, csrc/device_md.h: host and device code test the mask against them) and one in
Python (`api.DebugBit`, what the tests pass as Engine(debug=...)).  The two must be the same list: name by name, value by value."""
import os
import re

from aztotmd_amd import api

HEADER = os.path.join(os.path.dirname(os.path.abspath(api.__file__)), "csrc", "device_md.h")


def header_bits():
    text = open(HEADER).read()
    block = re.search(r"enum\s+DebugBit\b[^{]*\{(.*?)\};", text, re.S)
    assert block, "enum DebugBit not found in " + HEADER
    body = re.sub(r"//[^\n]*", "", block.group(1))
    entries = [e.strip() for e in body.split(",") if e.strip()]
    bits = {}
    for e in entries:
        m = re.fullmatch(r"(DBG_\w+)\s*=\s*(\d+)", e)
        assert m, "enum DebugBit: cannot read the entry %r" % e
        assert m.group(1) not in bits, m.group(1)
        bits[m.group(1)] = int(m.group(2))
    return bits


def test_python_names_match_the_header():
    cxx = header_bits()
    py = {name: int(member) for name, member in api.DebugBit.__members__.items()}      # (__members__ also lists aliases: a value used twice would show)
    assert len(cxx) >= 23
    assert sorted(py) == sorted(cxx)
    for name, value in cxx.items():
        assert py[name] == value, (name, py[name], value)


def test_switches_do_not_overlap():
    """every switch is one bit of its own, but for the two-bit build-phase field"""
    cxx = header_bits()
    seen = 0
    for name, value in cxx.items():
        assert value & seen == 0, name
        if name != "DBG_BUILD_PHASE_MASK":
            assert value & (value - 1) == 0, name
        seen |= value
