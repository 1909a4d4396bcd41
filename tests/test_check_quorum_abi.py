"""CPU: CheckQuorum's four exports and its message kind exist where a caller looks for them -- declared in include/raftq.h and
include/raftq_step.h, exported by the library, bound by the package and by the Go source -- validate their arguments without
touching a device, and the headers state the contract (the rules, the CHOICE marks, the 16-bit bound, what the switch closes)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("raftq_set_check_quorum", "raftq_load_activity", "raftq_read_activity", "raftq_collect_checks")


@pytest.fixture(scope="module")
def lib():
    from raftsql_amd import _lib, build

    build.build_lib()
    return _lib.load()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _flat(*parts):
    return " ".join(re.sub(r"\n[ \t]*\*(?!/)", "\n", _read(*parts)).split())


def _code(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_headers_declare_the_calls_and_the_kind():
    hdr = _code(_read("include", "raftq.h"))
    assert re.search(r"int\s+raftq_set_check_quorum\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert re.search(r"int\s+raftq_load_activity\s*\(\s*raftq_t\s*\*\s*h\s*,\s*const\s+uint16_t\s*\*\s*active\s*,\s*const\s+uint32_t\s*\*\s*lead_elapsed\s*\)\s*;", hdr)
    assert re.search(r"int\s+raftq_read_activity\s*\(\s*raftq_t\s*\*\s*h\s*,\s*uint16_t\s*\*\s*active\s*,\s*uint32_t\s*\*\s*lead_elapsed\s*\)\s*;", hdr)
    assert re.search(r"int\s+raftq_collect_checks\s*\(\s*raftq_t\s*\*\s*h\s*,\s*uint64_t\s*\*\s*groups\s*,\s*uint64_t\s+cap\s*,\s*uint64_t\s*\*\s*n\s*\)\s*;", hdr)
    assert re.search(r"#define\s+RAFTQ_MSG_CHECK_QUORUM\s+12\b", _code(_read("include", "raftq_step.h")))
    # raftq_tick_counts_t keeps its two fields
    assert re.search(r"typedef struct raftq_tick_counts \{\s*uint64_t n_hup;\s*uint64_t n_beat;\s*\} raftq_tick_counts_t;", hdr)


def test_library_exports_and_package_binds_them(lib):
    from raftsql_amd import _lib, step
    from raftsql_amd.engine import QuorumEngine

    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    for method in ("set_check_quorum", "load_activity", "read_activity", "collect_checks"):
        assert callable(getattr(QuorumEngine, method, None)), method
    assert step.MSG_CHECK_QUORUM == 12 and step.MSG_CHECK_QUORUM not in step.MSG_TYPES  # (the kinds every handle takes)


def test_go_source_binds_them():
    go = _read("go", "raftq", "raftq.go")
    assert re.search(r"func \(e \*Engine\) SetCheckQuorum\(on bool\) error", go) and "C.raftq_set_check_quorum(e.h, v)" in go
    assert re.search(r"func \(e \*Engine\) LoadActivity\(active \[\]uint16, leadElapsed \[\]uint32\) error", go) and "C.raftq_load_activity(e.h, a, l)" in go
    assert re.search(r"func \(e \*Engine\) ReadActivity\(active \[\]uint16, leadElapsed \[\]uint32\) error", go) and "C.raftq_read_activity(e.h, a, l)" in go
    assert re.search(r"func \(e \*Engine\) CollectChecks\(out \[\]uint64\) \(uint64, error\)", go) and "C.raftq_collect_checks(e.h, p, C.uint64_t(len(out)), &n)" in go
    assert "C.RAFTQ_MSG_CHECK_QUORUM" in _read("go", "raftq", "step.go")
    assert "SetCheckQuorum" in _read("go", "raftq", "README.md")


def test_null_handle_touches_no_device(lib):
    from raftsql_amd import _lib

    for on in (0, 1, 2):
        assert lib.raftq_set_check_quorum(None, on) == _lib.RAFTQ_EINVAL
    a, le, n = (C.c_uint16 * 4)(), (C.c_uint32 * 4)(), C.c_uint64(7)
    assert lib.raftq_load_activity(None, a, le) == _lib.RAFTQ_EINVAL
    assert lib.raftq_read_activity(None, a, le) == _lib.RAFTQ_EINVAL
    assert lib.raftq_collect_checks(None, None, 0, C.byref(n)) == _lib.RAFTQ_EINVAL and n.value == 7
    assert b"null handle" in lib.raftq_last_error(None)


def test_headers_state_the_contract():
    raftq_h, step_h = _flat("include", "raftq.h"), _flat("include", "raftq_step.h")
    tick = raftq_h[raftq_h.index("CheckQuorum: the leader's lease"):raftq_h.index("int raftq_campaign")]
    for said in ("PARITY UNPINNED", "CHOICE", "raftq_clone_state does not copy it", "65535", "popcount((active | 1 << self) & members)",
                 "action 3", "NO beat is raised this tick", "misses exactly one heartbeat", "raftq_collect_checks", "check quorum",
                 "raftq_tick_collect, raftq_tick_collect_lists", "raftq_tick_frames, raftq_tick_elect_frames", "raftq_set_tick",
                 "neither raftq_set_self nor raftq_load_node", "*n = 0 with the switch off", "raftq_tick_counts_t keeps its two fields"):
        assert said in tick, said
    assert "3: a leader's failed check" in raftq_h
    rules = step_h[step_h.index("CheckQuorum in Step"):step_h.index("raftq_msg_t._pad[1] once the handle opted in")]
    for said in ("PARITY UNPINNED", "CHOICE", "in front of the reject branch", "a non-voter's bit is stored and does not count", "reset()",
                 "inLease = role == leader || (lead != None && elapsed[g] < election_tick)", "RAFTQ_OUT_NONE, no state change, no response",
                 "a candidate has no lead", "RAFTQ_MSG_CHECK_QUORUM", "the 64-byte and the 40-byte record", "RAFTQ_OUTF_STEPPED_DOWN",
                 "no RAFTQ_OUTF_HARDSTATE", "An empty mask", "unknown kind that fails its batch", "raftq_node does not turn the switch on"):
        assert said in rules, said


def test_documents_name_it():
    design = _read("DESIGN.md")
    assert "raftq_set_check_quorum" in design and "tick_check_kernel" in design and "profiles/r24" in design
    assert "PreVote, CheckQuorum and leadership transfer are not modelled anywhere" not in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert "raftq_set_check_quorum" in _read(doc), doc
    assert os.path.exists(os.path.join(ROOT, "profiles", "r24", "README.md"))
