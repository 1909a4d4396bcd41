"""CPU: raftq_tick_set_voters exists where a caller looks for it -- declared in include/raftq.h, exported by the library, bound by
the package, by NodeEngine and by the Go source -- refuses a NULL handle without touching a device, and the headers state the
contract of Tick and its two device-built rounds over each group's own members."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "raftq_tick_set_voters"


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


def test_header_declares_the_switch():
    hdr = _code(_read("include", "raftq.h"))
    assert re.search(r"int\s+raftq_tick_set_voters\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", hdr)


def test_library_exports_and_package_binds_it(lib):
    from raftsql_amd import _lib
    from raftsql_amd.step import NodeEngine

    assert NAME in _lib.EXPORTS and hasattr(lib, NAME)
    assert callable(getattr(NodeEngine, "set_tick_voters", None))


def test_go_source_binds_it():
    go = _read("go", "raftq", "step.go")
    assert re.search(r"func \(e \*Engine\) SetTickVoters\(on bool\) error", go)
    assert "C.raftq_tick_set_voters(e.h, v)" in go
    assert "SetTickVoters" in _read("go", "raftq", "README.md")


def test_null_handle_touches_no_device(lib):
    from raftsql_amd import _lib

    for on in (0, 1, 2):
        assert lib.raftq_tick_set_voters(None, on) in (_lib.RAFTQ_EINVAL, _lib.RAFTQ_ENODEV)


def test_headers_state_the_contract():
    raftq_h, wire_h, step_h, node_h = (_flat("include", n) for n in ("raftq.h", "raftq_wire.h", "raftq_step.h", "raftq_node.h"))
    for name, text in (("raftq.h", raftq_h), ("raftq_wire.h", wire_h), ("raftq_step.h", step_h), ("raftq_node.h", node_h)):
        assert NAME in text, name
    # raftq.h: the voter-sets paragraph names the switch, the Tick section states promotable()'s rule
    sets = raftq_h[raftq_h.index("per-group voter sets"):raftq_h.index("typedef struct raftq_voter_delta")]
    assert NAME in sets and "raftq_tick_frames" in sets and "raftq_step_frames_respond" in sets
    tick = raftq_h[raftq_h.index("batched Tick (SURVEY.md"):raftq_h.index("#define RAFTQ_ROLE_FOLLOWER")]
    for words in ("promotable()", "r.elapsed = 0", "mine clear", "elapsed = 0, action 0", "raftq_clone_state does not copy it",
                  "raftq_load_voters(h, NULL) does not clear it", "Independent of raftq_step_set_voters", "RAFTQ_EINVAL", "RAFTQ_ESTATE"):
        assert words in tick, words
    # raftq_wire.h: both calls' contracts -- the membership rule, zero-length frames, n_msgs, the RAFTQ_ESTATE line
    beat = wire_h[wire_h.index("A node's heartbeat round"):wire_h.index("int raftq_tick_frames(")]
    for words in ("voters[g]", "POSITIONAL", "frame_off[k + 1] == frame_off[k]", "number of frames that have bytes",
                  "did not opt in with raftq_tick_set_voters", "still beats its members"):
        assert words in beat, words
    elect = wire_h[wire_h.index("raftq_tick_frames plus a node's election round"):wire_h.index("int raftq_tick_elect_frames(")]
    for words in ("RAFTQ_OUT_BECAME_LEADER", "NOT RAFTQ_OUTF_ANSWERED", "every member p != self", "zero length",
                  "number of frames that have bytes", "did not opt in with raftq_tick_set_voters"):
        assert words in elect, words
    # raftq_step.h: the two tick calls are refused unless this switch is on; promotable() is no longer "not modelled"
    refused = step_h[step_h.index("What stays refused"):step_h.index("int raftq_step_set_voters")]
    assert "unless raftq_tick_set_voters" in refused and "promotable() is not modelled" not in step_h
    # raftq_node.h: the node still never loads masks
    assert "never loads masks" in node_h
