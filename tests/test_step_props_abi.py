"""CPU: raftq_step_set_props exists where a caller looks for it -- declared in include/raftq_step.h with the two result types and
the message type, exported by the library, bound by the package, by NodeEngine and by the Go source -- refuses a NULL handle
without touching a device, and the headers no longer say that Step does not accept a MsgProp."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "raftq_step_set_props"


@pytest.fixture(scope="module")
def lib():
    from raftsql_amd import _lib, build

    build.build_lib()
    return _lib.load()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _code(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_header_declares_the_switch_and_the_constants():
    hdr = _code(_read("include", "raftq_step.h"))
    assert re.search(r"int\s+raftq_step_set_props\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", hdr)
    for name, value in (("RAFTQ_MSG_PROP", 2), ("RAFTQ_OUT_PROPOSED", 12), ("RAFTQ_OUT_FORWARD", 13)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
    # one definition in the headers a caller includes together (raftq_wire.h includes raftq_step.h)
    assert not re.search(r"#define\s+RAFTQ_MSG_PROP\b", _code(_read("include", "raftq_wire.h")))


def test_library_exports_and_package_binds_it(lib):
    from raftsql_amd import _lib, step
    from raftsql_amd.step import NodeEngine

    assert NAME in _lib.STEP_EXPORTS and hasattr(lib, NAME)
    assert callable(getattr(NodeEngine, "set_step_props", None))
    assert (step.MSG_PROP, step.OUT_PROPOSED, step.OUT_FORWARD) == (2, 12, 13)


def test_go_source_binds_it():
    go = _read("go", "raftq", "step.go")
    assert re.search(r"func \(e \*Engine\) SetStepProps\(on bool\) error", go)
    assert "C.raftq_step_set_props(e.h, v)" in go
    for name in ("C.RAFTQ_MSG_PROP", "C.RAFTQ_OUT_PROPOSED", "C.RAFTQ_OUT_FORWARD"):
        assert name in go, name
    assert "SetStepProps" in _read("go", "raftq", "README.md")
    assert "TestStepPropsAgainstEtcd" in _read("go", "raftq", "etcd_pin_test.go")
    assert "TestStepPropsTable" in _read("go", "raftq", "step_tables_test.go")


def test_null_handle_touches_no_device(lib):
    from raftsql_amd import _lib

    for on in (0, 1, 2):
        assert lib.raftq_step_set_props(None, on) in (_lib.RAFTQ_EINVAL, _lib.RAFTQ_ENODEV)


def test_headers_state_the_contract():
    step_h = " ".join(_read("include", "raftq_step.h").split())
    assert "not accepted" not in step_h
    assert "MsgProp / MsgSnap" not in step_h
    for said in (NAME, "RAFTQ_OUT_PROPOSED", "RAFTQ_OUT_FORWARD", "lead - 1", "raftq_step_submit_wire", "raftq_msg40_t", "2^64", "CHOICE",
                 "raftq_clone_state does not copy it"):
        assert said in step_h[step_h.index("Step takes forwarded proposals"):], said
    wire_h = " ".join(_read("include", "raftq_wire.h").split())
    assert NAME in wire_h and "RAFTQ_OUT_PROPOSED" in wire_h


def test_design_no_longer_lists_msgprop_among_the_callers():
    design = _read("DESIGN.md")
    assert NAME in design and "profiles/r21" in design
    assert NAME in _read("INTEGRATION.md")
    assert os.path.exists(os.path.join(ROOT, "profiles", "r21", "README.md"))
