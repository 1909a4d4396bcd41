"""CPU: raftq_set_create_voters exists where a caller looks for it -- declared in include/raftq.h, exported by the library, bound
by the package (SweepSet(engines, voters=True)) and by the Go source -- validates its arguments without touching a device, and the
headers no longer say that a sweep set cannot hold a masked member."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "raftq_set_create_voters"


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


def test_header_declares_the_constructor():
    hdr = _code(_read("include", "raftq.h"))
    assert re.search(r"int\s+raftq_set_create_voters\s*\(\s*raftq_t\s*\*\s*const\s*\*\s*handles\s*,\s*uint32_t\s+n\s*,\s*raftq_set_t\s*\*\*\s*out\s*\)\s*;", hdr)
    # the scanner of tests/test_abi.py reads names without digits: this one is seen by it
    assert not re.search(r"\d", NAME)


def test_library_exports_and_package_binds_it(lib):
    from raftsql_amd import _lib
    from raftsql_amd.engine import SweepSet

    assert NAME in _lib.EXPORTS and hasattr(lib, NAME)
    sig = inspect.signature(SweepSet.__init__)
    assert "voters" in sig.parameters and sig.parameters["voters"].default is False


def test_go_source_binds_it():
    go = _read("go", "raftq", "raftq.go")
    assert re.search(r"func NewSetVoters\(members \[\]\*Engine\) \(\*Set, error\)", go)
    assert "raftq_set_create_voters(hs, n, out)" in go
    assert "NewSetVoters" in _read("go", "raftq", "README.md")


def test_argument_validation_without_device(lib):
    from raftsql_amd import _lib

    out = C.c_void_p(0xdead)
    assert lib.raftq_set_create_voters(None, 0, C.byref(out)) == _lib.RAFTQ_EINVAL
    assert out.value is None  # *out is cleared before anything else is looked at
    assert b"raftq_set_create_voters" in lib.raftq_set_last_error(None)
    out = C.c_void_p(0xdead)
    assert lib.raftq_set_create_voters(None, 3, C.byref(out)) == _lib.RAFTQ_EINVAL and out.value is None
    assert lib.raftq_set_create_voters(None, 3, None) == _lib.RAFTQ_EINVAL
    arr = (C.c_void_p * 2)(None, None)
    out = C.c_void_p(0xdead)
    assert lib.raftq_set_create_voters(arr, 2, C.byref(out)) == _lib.RAFTQ_EINVAL and out.value is None  # a null member


def test_headers_state_the_contract():
    raftq_h, step_h = _flat("include", "raftq.h"), _flat("include", "raftq_step.h")
    for gone in ("Not built, and refused with RAFTQ_ESTATE", "set members cannot hold masks", "Sweep sets with a masked member and"):
        assert gone not in raftq_h and gone not in step_h, gone
    sets = raftq_h[raftq_h.index("per-group voter sets"):raftq_h.index("typedef struct raftq_voter_delta")]
    assert NAME in sets and "raftq_set_create refuses a masked handle" in sets
    tick = raftq_h[raftq_h.index("batched Tick (SURVEY.md"):raftq_h.index("#define RAFTQ_ROLE_FOLLOWER")]
    assert NAME in tick and "raftq_set_tick" in tick
    sweep_sets = raftq_h[raftq_h.index("sweep sets: many handles, one dispatch"):raftq_h.index("typedef struct raftq_set raftq_set_t")]
    for words in (NAME, "members with and without masks may be mixed", "raftq_load_voters (NULL included)", "raftq_step_async(member, flags)",
                  "launches exactly what a plain set launches", "there is no persistent masked walk", "RAFTQ_SWEEP_LDS stays refused",
                  "promotable()", "RAFTQ_TICK_SHAPE does not apply", "no member has ticked"):
        assert words in sweep_sets, words
    assert NAME in step_h
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        assert NAME in _read(doc), doc
