"""CPU: raftq_propose_set_forward and raftq_propose_outcomes exist where a caller looks for them -- declared in include/raftq_wire.h
with the three RAFTQ_PROP_* constants, exported by the library, bound by the package, by WireEngine and by the Go source --, refuse a
NULL handle without touching a device, and the header states the contract."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH, OUTCOMES = "raftq_propose_set_forward", "raftq_propose_outcomes"
CONSTANTS = {"RAFTQ_PROP_APPENDED": 0, "RAFTQ_PROP_FORWARDED": 1, "RAFTQ_PROP_DROPPED": 2}


@pytest.fixture(scope="module")
def lib():
    from raftsql_amd import _lib, build

    build.build_lib()
    return _lib.load()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _flat(*parts):
    """the file as one line, the comment blocks' leading ` * ` taken out: a phrase may run over a line break"""
    return " ".join(re.sub(r"\n[ \t]*\*(?!/)", "\n", _read(*parts)).split())


def _code(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _define(name):
    m = re.search(r"#define\s+%s\s+(\d+)u?\b" % name, _read("include", "raftq_wire.h"))
    assert m, name
    return int(m.group(1))


def test_header_declares_the_two_calls_and_the_three_constants():
    hdr = _code(_read("include", "raftq_wire.h"))
    assert re.search(r"int\s+raftq_propose_set_forward\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert re.search(r"int\s+raftq_propose_outcomes\s*\(\s*raftq_t\s*\*\s*h\s*,\s*const\s+uint8_t\s*\*\*\s*what\s*,\s*uint64_t\s*\*\s*n\s*\)\s*;", hdr)
    assert hdr.index("int raftq_propose_frames") < hdr.index("int raftq_bcast_set_voters") < hdr.index(SWITCH) < hdr.index(OUTCOMES)
    for name, value in CONSTANTS.items():
        assert _define(name) == value


def test_library_exports_and_package_binds_them(lib):
    from raftsql_amd import _lib
    from raftsql_amd import wire as W

    for name in (SWITCH, OUTCOMES):
        assert name in _lib.WIRE_EXPORTS and hasattr(lib, name)
    assert callable(getattr(W.WireEngine, "set_propose_forward", None)) and callable(getattr(W.WireEngine, "propose_outcomes", None))
    assert (W.PROP_APPENDED, W.PROP_FORWARDED, W.PROP_DROPPED) == tuple(_define(k) for k in CONSTANTS)
    assert W.WireEngine._propose_forward is False  # off by default


def test_go_source_binds_them():
    go = "".join(_read("go", "raftq", f) for f in sorted(os.listdir(os.path.join(ROOT, "go", "raftq"))) if f.endswith(".go"))
    assert re.search(r"func \(e \*Engine\) SetProposeForward\(on bool\) error", go)
    assert "C.raftq_propose_set_forward(e.h, v)" in go and "C.raftq_propose_outcomes(e.h, &what, &nWhat)" in go
    assert re.search(r"func \(e \*Engine\) ProposeFrames\([^)]*\) \(need uint64, outcomes \[\]byte, err error\)", go)
    for name, value in (("PropAppended", 0), ("PropForwarded", 1), ("PropDropped", 2)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, value), go)
    assert "SetProposeForward" in _read("go", "raftq", "README.md")


def test_null_handle_touches_no_device(lib):
    from raftsql_amd import _lib

    for on in (0, 1, 2):
        assert lib.raftq_propose_set_forward(None, on) in (_lib.RAFTQ_EINVAL, _lib.RAFTQ_ENODEV)
    p, n = C.c_void_p(None), C.c_uint64(7)
    assert lib.raftq_propose_outcomes(None, C.byref(p), C.byref(n)) in (_lib.RAFTQ_EINVAL, _lib.RAFTQ_ENODEV)


def test_header_states_the_contract():
    wire_h = _flat("include", "raftq_wire.h")
    call = wire_h[wire_h.index("A follower's proposals (raftq_propose_set_forward(h, 1), below)"):wire_h.index("typedef struct raftq_prop {")]
    for words in ("m.To = r.lead; r.send(m)", "MsgProp{To: lead - 1, From: self, Group: g, Term: 0", "raft.send leaves a MsgProp's Term alone",
                  "Term: 0, Index: 0, Data", "an entry with data_len == 0 has no Data field", "Nothing of the group's state changes",
                  "RAFTQ_PROP_APPENDED", "RAFTQ_PROP_FORWARDED", "RAFTQ_PROP_DROPPED", "no leader; dropping proposal", "lead - 1 == self", "CHOICE",
                  "One call may mix all three", "a group named twice", "A refused call applies nothing", "POSITIONAL",
                  "n_msgs + (N - 1) * n_props + 1 entries", "only in the run of its leader's slot", "frames of ZERO length",
                  "The entry headers are written for every record", "counts->n_msgs is n_msgs plus the frames that have bytes",
                  "all dropped succeeds", "whether or not lead or self is a member", "judged for leader records only"):
        assert words in call, words
    sw = wire_h[wire_h.index("raftq_propose_frames for a node that does not lead every group"):wire_h.index("int raftq_propose_set_forward(")]
    for words in ("0, the default", "this node does not lead its group", "RAFTQ_EINVAL", "RAFTQ_ESTATE", "NULL handle",
                  "raftq_clone_state does not copy it", "Only raftq_propose_frames reads it", "raftq_node does not turn it on", "RAFTQ_OUT_FORWARD"):
        assert words in sw, words
    oc = wire_h[wire_h.index("What became of every record of the last raftq_propose_frames call"):wire_h.index("int raftq_propose_outcomes(")]
    for words in ("SUCCEEDED", "memory the handle owns", "valid until the next call on the handle", "single wait", "packed by the wave",
                  "*n = 0", "NULL handle"):
        assert words in oc, words
