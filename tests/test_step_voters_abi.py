"""CPU: raftq_step_set_voters exists where a caller looks for it -- declared in include/raftq_step.h, exported by the library,
bound by the package, by NodeEngine and by the Go source -- refuses a NULL handle without touching a device, and the headers
no longer say that every Step entry point refuses a masked handle."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "raftq_step_set_voters"


@pytest.fixture(scope="module")
def lib():
    from raftsql_amd import _lib, build

    build.build_lib()
    return _lib.load()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _code(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_header_declares_the_switch():
    hdr = _code(_read("include", "raftq_step.h"))
    assert re.search(r"int\s+raftq_step_set_voters\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", hdr)


def test_library_exports_and_package_binds_it(lib):
    from raftsql_amd import _lib
    from raftsql_amd.step import NodeEngine

    assert NAME in _lib.STEP_EXPORTS and hasattr(lib, NAME)
    assert callable(getattr(NodeEngine, "set_step_voters", None))


def test_go_source_binds_it():
    go = _read("go", "raftq", "step.go")
    assert re.search(r"func \(e \*Engine\) SetStepVoters\(on bool\) error", go)
    assert "C.raftq_step_set_voters(e.h, v)" in go
    assert "SetStepVoters" in _read("go", "raftq", "README.md")


def test_null_handle_touches_no_device(lib):
    from raftsql_amd import _lib

    for on in (0, 1, 2):
        assert lib.raftq_step_set_voters(None, on) in (_lib.RAFTQ_EINVAL, _lib.RAFTQ_ENODEV)


def test_headers_state_the_contract():
    """the "not built" paragraphs: Step is no longer in them, the device-built broadcasts still are"""
    for name in ("raftq.h", "raftq_step.h", "raftq_wire.h", "raftq_node.h"):
        text = " ".join(_read("include", name).split())
        assert "every entry point of raftq_step.h / raftq_wire.h that runs Step's maybeCommit or poll on the device" not in text, name
        assert NAME in text, name
    step_h = " ".join(_read("include", "raftq_step.h").split())
    for still in ("raftq_step_frames_respond", "raftq_propose_frames", "raftq_tick_frames", "raftq_tick_elect_frames"):
        assert still in step_h[step_h.index("What stays refused"):], still
