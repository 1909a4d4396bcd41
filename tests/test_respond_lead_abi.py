"""CPU: raftq_respond_set_lead exists where a caller looks for it -- declared in include/raftq_wire.h, exported by the library, bound
by the package, by WireEngine and by the Go source -- refuses a NULL handle without touching a device, and
RAFTQ_RESPOND_LEAD_FRAME_MAX is what the marshal makes of the largest frame the switch adds."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "raftq_respond_set_lead"


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


def test_header_declares_the_switch():
    hdr = _code(_read("include", "raftq_wire.h"))
    assert re.search(r"int\s+raftq_respond_set_lead\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert hdr.index("raftq_bcast_set_voters") < hdr.index(NAME)  # beside the other switch of the call


def test_library_exports_and_package_binds_it(lib):
    from raftsql_amd import _lib
    from raftsql_amd.wire import WireEngine

    assert NAME in _lib.WIRE_EXPORTS and hasattr(lib, NAME)
    assert callable(getattr(WireEngine, "set_respond_lead", None))


def test_go_source_binds_it():
    go = "".join(_read("go", "raftq", f) for f in sorted(os.listdir(os.path.join(ROOT, "go", "raftq"))) if f.endswith(".go"))
    assert re.search(r"func \(e \*Engine\) SetRespondLead\(on bool\) error", go)
    assert "C.raftq_respond_set_lead(e.h, v)" in go
    assert re.search(r"RespondLeadFrameMax\s*=\s*%d\b" % _define("RAFTQ_RESPOND_LEAD_FRAME_MAX"), go)
    assert "SetRespondLead" in _read("go", "raftq", "README.md")


def test_null_handle_touches_no_device(lib):
    from raftsql_amd import _lib

    for on in (0, 1, 2):
        assert lib.raftq_respond_set_lead(None, on) in (_lib.RAFTQ_EINVAL, _lib.RAFTQ_ENODEV)


def test_the_bound_is_the_marshal_of_the_largest_frame():
    """a MsgApp with one empty entry and every varint at its widest -- term, logTerm, index, commit, group and the entry's term and
    index at 2^64 - 1 (ten bytes each); type, to, from and the entry's type are one byte whatever they hold (raftpb types <= 9, raft
    IDs <= 9, EntryNormal / EntryConfChange) -- marshalled by the oracle's encoder"""
    from oracle import pywire
    from raftsql_amd import wire as W

    big = np.uint64(2**64 - 1)
    m = np.zeros(1, W.WIRE_MSG_DT)
    m["type"], m["to"], m["from"], m["n_ents"] = 3, 8, 7, 1
    for k in ("term", "log_term", "index", "commit", "group"):
        m[k] = big
    e = np.zeros(1, W.WIRE_ENT_DT)
    e["term"], e["index"] = big, big
    bound = _define("RAFTQ_RESPOND_LEAD_FRAME_MAX")
    for etype in (0, 1):
        e["type"] = etype
        s, off = pywire.wire_encode(m, e, np.zeros(1, np.uint8))
        assert len(s) == bound == W.RESPOND_LEAD_FRAME_MAX, (etype, len(s))
    # the entries field alone: tag + length, the tags of type / term / index, one byte + ten + ten
    assert bound == _define("RAFTQ_RESPOND_FRAME_MAX") + (2 + 3 + 1 + 10 + 10)
    assert bound > _define("RAFTQ_RESPOND_FRAME_MAX") == W.RESPOND_FRAME_MAX


def test_respond_cap_follows_the_switch():
    """(no device: the engine's word alone)"""
    from raftsql_amd import wire as W

    e = W.WireEngine.__new__(W.WireEngine)
    e.n_peers = 5
    assert e.respond_cap(7) == 7 * 4 * W.RESPOND_FRAME_MAX
    e._respond_lead = True
    assert e.respond_cap(7) == 7 * 4 * W.RESPOND_LEAD_FRAME_MAX


def test_header_states_the_contract():
    wire_h = _flat("include", "raftq_wire.h")
    resp = wire_h[wire_h.index("raftq_step_frames + the messages its results call for"):wire_h.index("#define RAFTQ_OUTF_ANSWERED")]
    for words in ("becomeLeader's broadcast", "lastTerm as it stood BEFORE becomeLeader", "Index: lastIndex - 1", "does not end the prefix",
                  "at_tail == NULL", "RAFTQ_RESPOND_LEAD_FRAME_MAX", "never exist in host memory", "unless raftq_respond_set_lead"):
        assert words in resp, words
    sw = wire_h[wire_h.index("raftq_step_frames_respond's fifth kind"):wire_h.index("int raftq_respond_set_lead(")]
    for words in ("RAFTQ_EINVAL", "RAFTQ_ESTATE", "NULL handle", "raftq_clone_state does not copy it", "the default", "raftq_tick_elect_frames"):
        assert words in sw, words
