"""CPU: raftq_bcast_set_voters exists where a caller looks for it -- declared in include/raftq_wire.h, exported by the library,
bound by the package, by WireEngine and by the Go source -- refuses a NULL handle without touching a device, and the headers
state the contract of the two device-built broadcasts over each group's own members."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "raftq_bcast_set_voters"


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
    hdr = _code(_read("include", "raftq_wire.h"))
    assert re.search(r"int\s+raftq_bcast_set_voters\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", hdr)


def test_library_exports_and_package_binds_it(lib):
    from raftsql_amd import _lib
    from raftsql_amd.wire import WireEngine

    assert NAME in _lib.WIRE_EXPORTS and hasattr(lib, NAME)
    assert callable(getattr(WireEngine, "set_bcast_voters", None))


def test_go_source_binds_it():
    go = "".join(_read("go", "raftq", f) for f in sorted(os.listdir(os.path.join(ROOT, "go", "raftq"))) if f.endswith(".go"))
    assert re.search(r"func \(e \*Engine\) SetBcastVoters\(on bool\) error", go)
    assert "C.raftq_bcast_set_voters(e.h, v)" in go
    assert "SetBcastVoters" in _read("go", "raftq", "README.md")


def test_null_handle_touches_no_device(lib):
    from raftsql_amd import _lib

    for on in (0, 1, 2):
        assert lib.raftq_bcast_set_voters(None, on) in (_lib.RAFTQ_EINVAL, _lib.RAFTQ_ENODEV)


def test_headers_state_the_contract():
    raftq_h, wire_h, step_h, node_h = (_flat("include", n) for n in ("raftq.h", "raftq_wire.h", "raftq_step.h", "raftq_node.h"))
    for name, text in (("raftq.h", raftq_h), ("raftq_wire.h", wire_h), ("raftq_step.h", step_h), ("raftq_node.h", node_h)):
        assert NAME in text, name
    # raftq.h: the voter-sets paragraph names the switch and still names the calls
    sets = raftq_h[raftq_h.index("per-group voter sets"):raftq_h.index("typedef struct raftq_voter_delta")]
    assert NAME in sets and "raftq_tick_frames" in sets and "raftq_step_frames_respond" in sets and "raftq_propose_frames" in sets
    # raftq_wire.h: the switch's own paragraph
    sw = wire_h[wire_h.index("The switch of the two calls above"):wire_h.index("int raftq_bcast_set_voters(")]
    for words in ("RAFTQ_EINVAL", "RAFTQ_ESTATE", "voter masks", "raftq_clone_state does not copy it", "raftq_load_voters(h, NULL) does not clear it",
                  "Independent of raftq_tick_set_voters", "NULL handle"):
        assert words in sw, words
    # ... the respond call's contract over members
    resp = wire_h[wire_h.index("raftq_step_frames + the messages its results call for"):wire_h.index("#define RAFTQ_OUTF_ANSWERED")]
    for words in ("voters[g]", "whoever sent", "COMPACT", "ZERO frames", "RAFTQ_OUTF_ANSWERED", "did not opt in with raftq_bcast_set_voters",
                  "whether or not that switch is on"):
        assert words in resp, words
    # ... and the proposals': positional, the two refusals, the recipe
    prop = wire_h[wire_h.index("A node's OUTBOUND half of a turn"):wire_h.index("typedef struct raftq_prop {")]
    for words in ("POSITIONAL", "frame_off[k + 1] == frame_off[k]", "number of frames that have bytes", "no member of its group",
                  "would move the commit index", "raftq_apply_log_deltas", "UNCHANGED tail", "did not opt in with raftq_bcast_set_voters"):
        assert words in prop, words
    # raftq_step.h: what stays refused, and unless what
    refused = step_h[step_h.index("What stays refused"):step_h.index("int raftq_step_set_voters")]
    for words in ("raftq_step_frames_respond", "raftq_propose_frames", "raftq_tick_frames", "raftq_tick_elect_frames", "unless raftq_tick_set_voters",
                  "unless raftq_bcast_set_voters"):
        assert words in refused, words
    # raftq_node.h: the node still never loads masks
    assert "never loads masks" in node_h
