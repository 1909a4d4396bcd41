"""CPU: raftq_respond_set_props exists where a caller looks for it -- declared in include/raftq_wire.h, exported by the library, bound
by the package, by WireEngine and by the Go source -- refuses a NULL handle without touching a device, RAFTQ_RESPOND_ENT_MAX is what
the header derives, and both headers state the contract."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "raftq_respond_set_props"


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


def test_header_declares_the_switch_and_the_constant():
    hdr = _code(_read("include", "raftq_wire.h"))
    assert re.search(r"int\s+raftq_respond_set_props\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert hdr.index("raftq_respond_set_lead") < hdr.index(NAME)  # beside the other switch of the call
    # the entries field's tag and length, four tags, a five-byte type, term and index of ten, a five-byte data length
    assert _define("RAFTQ_RESPOND_ENT_MAX") == (1 + 5) + 4 + 5 + 10 + 10 + 5 == 40


def test_library_exports_and_package_binds_it(lib):
    from raftsql_amd import _lib
    from raftsql_amd import wire as W

    assert NAME in _lib.WIRE_EXPORTS and hasattr(lib, NAME)
    assert callable(getattr(W.WireEngine, "set_respond_props", None))
    assert W.RESPOND_ENT_MAX == _define("RAFTQ_RESPOND_ENT_MAX")


def test_go_source_binds_it():
    go = "".join(_read("go", "raftq", f) for f in sorted(os.listdir(os.path.join(ROOT, "go", "raftq"))) if f.endswith(".go"))
    assert re.search(r"func \(e \*Engine\) SetRespondProps\(on bool\) error", go)
    assert "C.raftq_respond_set_props(e.h, v)" in go
    assert re.search(r"RespondEntMax\s*=\s*%d\b" % _define("RAFTQ_RESPOND_ENT_MAX"), go)
    assert "SetRespondProps" in _read("go", "raftq", "README.md")
    assert "TestRespondPropsAgainstEtcd" in _read("go", "raftq", "respond_props_pin_test.go")


def test_null_handle_touches_no_device(lib):
    from raftsql_amd import _lib

    for on in (0, 1, 2):
        assert lib.raftq_respond_set_props(None, on) in (_lib.RAFTQ_EINVAL, _lib.RAFTQ_ENODEV)


def test_respond_cap_follows_the_switch():
    """(no device: the engine's words alone)"""
    from raftsql_amd import wire as W

    e = W.WireEngine.__new__(W.WireEngine)
    e.n_peers = 5
    assert e.respond_cap(7, 1000, 30) == 7 * 4 * W.RESPOND_FRAME_MAX
    e._respond_props = True
    assert e.respond_cap(7, 1000, 30) == 7 * 4 * W.RESPOND_FRAME_MAX + 4 * (1000 + 30 * 40)
    e._respond_lead = True
    assert e.respond_cap(7, 1000, 30) == 7 * 4 * W.RESPOND_LEAD_FRAME_MAX + 4 * (1000 + 30 * 40)


def test_headers_state_the_contract():
    wire_h = _flat("include", "raftq_wire.h")
    resp = wire_h[wire_h.index("raftq_step_frames + the messages its results call for"):wire_h.index("#define RAFTQ_OUTF_ANSWERED")]
    for words in ("A forwarded proposal's MsgApps", "Index: lastIndex BEFORE the proposal", "LogTerm: lastTerm BEFORE the proposal",
                  "Commit: committed AFTER the message", "Index: old lastIndex + 1 + k", "The at_tail bit STAYS set", "the prefix does not end",
                  "the pool the inbound stream", "ents != NULL", "cap >= n * (N - 1) * FRAME + (N - 1) * (nbytes + ents_cap * RAFTQ_RESPOND_ENT_MAX)",
                  "6 + 4 + 5 + 20 + 5 = 40", "never exist in host memory", "unless raftq_respond_set_props", "RAFTQ_OUT_FORWARD stays the host's"):
        assert words in resp, words
    sw = wire_h[wire_h.index("raftq_step_frames_respond's sixth kind"):wire_h.index("int raftq_respond_set_props(")]
    for words in ("RAFTQ_EINVAL", "RAFTQ_ESTATE", "NULL handle", "raftq_clone_state does not copy it", "the default", "raftq_step_set_props",
                  "all eight combinations", "raftq_node does not turn it on"):
        assert words in sw, words
    step_h = _flat("include", "raftq_step.h")
    assert "builds no commit broadcast for the group" in step_h and "unless raftq_respond_set_props" in step_h
