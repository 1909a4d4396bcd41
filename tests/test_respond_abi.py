"""CPU: raftq_step_frames_respond (include/raftq_wire.h) is declared, bound and exported, refuses without a device, and its
result flag and frame bound are what the header, the Python binding and the Go binding say.  No compute is called here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from raftsql_amd import _lib, build

    build.build_lib()
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "raftq_wire.h")).read()


def _define(text, name):
    m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)u?\b" % name, text)
    assert m, name
    return int(m.group(1), 0)


def test_the_call_is_declared_bound_and_exported(lib):
    from raftsql_amd import _lib

    assert "raftq_step_frames_respond" in _lib.WIRE_EXPORTS
    assert hasattr(lib, "raftq_step_frames_respond")
    sig = dict((s[0], s[2]) for s in _lib._WIRE_SIGS)["raftq_step_frames_respond"]
    assert len(sig) == 16


def test_refuses_without_a_handle(lib):
    from raftsql_amd import _lib

    wc = _lib.WireCounts()
    rc = lib.raftq_step_frames_respond(None, None, 0, None, 0, 1, None, None, 0, None, None, 0, None, None, C.byref(wc), C.byref(wc))
    assert rc in (_lib.RAFTQ_EINVAL, _lib.RAFTQ_ENODEV)


def test_answered_flag_is_a_bit_of_its_own():
    from raftsql_amd import step as S
    from raftsql_amd import wire as W

    h = _header()
    step_h = open(os.path.join(ROOT, "include", "raftq_step.h")).read()
    others = [_define(step_h, n) for n in ("RAFTQ_OUTF_HARDSTATE", "RAFTQ_OUTF_COMMITTED", "RAFTQ_OUTF_UPDATED", "RAFTQ_OUTF_STEPPED_DOWN")]
    answered = _define(h, "RAFTQ_OUTF_ANSWERED")
    assert answered == W.OUTF_ANSWERED == 0x10
    assert bin(answered).count("1") == 1 and all(answered & o == 0 for o in others)
    assert answered & (S.OUTF_HARDSTATE | S.OUTF_COMMITTED | S.OUTF_UPDATED | S.OUTF_STEPPED_DOWN) == 0
    go = open(os.path.join(ROOT, "go", "raftq", "wire.go")).read()
    assert re.search(r"OutfAnswered\s*=\s*0x10\b", go)


def test_frame_bound_is_the_largest_payload_free_frame():
    """8-byte length; tags of type, to, from, term, logTerm, index (6 bytes); type / to / from take one byte each (type <= 9,
    raft IDs <= 9); term, logTerm, index, commit and group ten; commit tag, the empty snapshot (10), reject (2), rejectHint
    (tag + a zero), group tag -- what msg_head_size + msg_tail_size (raftq_wire_kernels.hpp) give at their largest"""
    from raftsql_amd import wire as W

    want = 8 + (6 + 1 + 1 + 1 + 10 + 10 + 10) + (1 + 10 + 10 + 2 + 1 + 1 + 1 + 10)
    assert _define(_header(), "RAFTQ_RESPOND_FRAME_MAX") == W.RESPOND_FRAME_MAX == want == 83
    go = open(os.path.join(ROOT, "go", "raftq", "wire.go")).read()
    assert re.search(r"RespondFrameMax\s*=\s*83\b", go)


def test_the_bound_holds_against_the_python_marshal():
    """the largest message the call builds, marshalled by the oracle's encoder, is exactly the bound"""
    import numpy as np

    from oracle import pywire
    from raftsql_amd import wire as W

    m = np.zeros(1, W.WIRE_MSG_DT)
    m["type"], m["to"], m["from"] = 3, 8, 7
    for k in ("term", "log_term", "index", "commit", "group"):
        m[k] = np.uint64(2**64 - 1)
    s, off = pywire.wire_encode(m, np.zeros(0, W.WIRE_ENT_DT), np.zeros(1, np.uint8))
    assert len(s) == W.RESPOND_FRAME_MAX
