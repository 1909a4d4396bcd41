"""CPU: PreVote's export, its two message kinds, its three result kinds and its role exist where a caller looks for them -- declared
in include/raftq.h and include/raftq_step.h, exported by the library, bound by the package and by the Go source --, the call
validates a NULL handle without touching a device, no record changed size, and the headers and documents state the contract."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFINES = {"RAFTQ_MSG_PRE_VOTE": 17, "RAFTQ_MSG_PRE_VOTE_RESP": 18, "RAFTQ_OUT_PRE_CAMPAIGN": 14, "RAFTQ_OUT_PRE_VOTE_RESP": 15,
           "RAFTQ_OUT_TERM_RESP": 16}


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


def test_headers_declare_the_call_and_the_constants():
    hdr, step_h = _code(_read("include", "raftq.h")), _code(_read("include", "raftq_step.h"))
    assert re.search(r"int\s+raftq_set_pre_vote\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert re.search(r"#define\s+RAFTQ_ROLE_PRE_CANDIDATE\s+3\b", hdr)
    for name, value in DEFINES.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), step_h), name
    # the values that were there keep theirs
    for name, value in (("RAFTQ_MSG_VOTE", 5), ("RAFTQ_MSG_CHECK_QUORUM", 12), ("RAFTQ_OUT_FORWARD", 13), ("RAFTQ_OUT_CAMPAIGN", 3)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), step_h), name
    assert re.search(r"#define\s+RAFTQ_ROLE_LEADER\s+2\b", hdr)


def test_record_sizes_are_unchanged():
    from raftsql_amd import step

    assert (step.MSG_DT.itemsize, step.MSG40_DT.itemsize, step.OUT_DT.itemsize, step.OUT_C_DT.itemsize, step.OUT_S_DT.itemsize) == (64, 40, 64, 40, 32)
    from tests.test_go_binding import c_structs, layout

    cs = c_structs()
    for struct, size in (("raftq_msg", 64), ("raftq_msg40", 40), ("raftq_step_out", 64), ("raftq_step_out_c", 40), ("raftq_step_out_s", 32)):
        assert layout(cs[struct])[1] == size, struct


def test_library_exports_and_package_binds_them(lib):
    from raftsql_amd import _lib, step
    from raftsql_amd.engine import QuorumEngine

    assert "raftq_set_pre_vote" in _lib.EXPORTS and hasattr(lib, "raftq_set_pre_vote")
    assert callable(getattr(QuorumEngine, "set_pre_vote", None))
    assert (step.MSG_PRE_VOTE, step.MSG_PRE_VOTE_RESP) == (17, 18) and step.MSG_PRE_VOTE not in step.MSG_TYPES  # (the kinds every handle takes)
    assert (step.OUT_PRE_CAMPAIGN, step.OUT_PRE_VOTE_RESP, step.OUT_TERM_RESP, step.ROLE_PRE_CANDIDATE) == (14, 15, 16, 3)


def test_go_source_binds_them():
    go, step_go = _read("go", "raftq", "raftq.go"), _read("go", "raftq", "step.go")
    assert re.search(r"func \(e \*Engine\) SetPreVote\(on bool\) error", go) and "C.raftq_set_pre_vote(e.h, v)" in go
    for name in DEFINES:
        assert "C." + name in step_go, name
    assert "SetPreVote" in _read("go", "raftq", "README.md")
    assert "PreVote" in _read("go", "raftq", "PIN.md")


def test_null_handle_touches_no_device(lib):
    from raftsql_amd import _lib

    for on in (0, 1, 2):
        assert lib.raftq_set_pre_vote(None, on) == _lib.RAFTQ_EINVAL
    assert b"null handle" in lib.raftq_last_error(None)


def test_the_compact_expanders_know_the_pre_campaign():
    """raftsql_amd.step.expand_compact / expand_short recover a RAFTQ_OUT_PRE_CAMPAIGN as they recover a RAFTQ_OUT_CAMPAIGN"""
    import numpy as np

    from raftsql_amd import step

    m = step.pack_msgs([3], step.MSG_HUP)
    c = np.zeros(1, step.OUT_C_DT)
    c["term"], c["index"], c["commit"], c["aux"], c["type"], c["role"] = 5, 7, 2, 4, step.OUT_PRE_CAMPAIGN, 3
    o = step.expand_compact(m, c)[0]
    assert (int(o["log_term"]), int(o["last_index"]), int(o["commit"]), int(o["index"])) == (4, 7, 2, 7)
    s = np.zeros(1, step.OUT_S_DT)
    s["term"], s["index"], s["commit"], s["type"], s["role"] = 5, 7, 4, step.OUT_PRE_CAMPAIGN, 3
    o = step.expand_short(m, s, np.full(4, 7, np.uint64), np.full(4, 2, np.uint64))[0]
    assert (int(o["log_term"]), int(o["last_index"]), int(o["commit"]), int(o["index"])) == (4, 7, 2, 7)


def test_headers_state_the_contract():
    raftq_h, step_h = _flat("include", "raftq.h"), _flat("include", "raftq_step.h")
    switch = raftq_h[raftq_h.index("PreVote: pre-elections"):raftq_h.index("int raftq_set_pre_vote")]
    for said in ("PARITY UNPINNED", "CHOICE: it requires CheckQuorum", "check quorum", "pre vote", "Upstream's two options are independent",
                 "raftq_clone_state does not copy it", "RAFTQ_ROLE_PRE_CANDIDATE", "tests role == 2 alone", "a follower without a leader",
                 "raftq_tick_elect_frames", "raftq_campaign stays the real becomeCandidate", "raftq_node does not turn the switch on",
                 "no device is touched"):
        assert said in switch, said
    rules = step_h[step_h.index("PreVote in Step"):step_h.index("raftq_msg_t._pad[1] once the handle opted in")]
    for said in ("PARITY UNPINNED", "CHOICE", "unknown kinds that fail their batch", "becomePreCandidate", "zeroed as Step's MsgHup always has",
                 "no RAFTQ_OUTF_HARDSTATE", "byte for byte what MsgHup gives without the switch", "recorded but not counted",
                 "ignored exactly as a MsgVote is", "becomeFollower(m.Term, None)", "RAFTQ_OUT_TERM_RESP", "holds nobody up",
                 "grant = (Vote == None || m.Term > r.Term || Vote == from + 1) && isUpToDate(m.Index, m.LogTerm)", "NOTHING changes",
                 "it polls MsgPreVoteResp and ignores MsgVoteResp", "RAFTQ_OUTF_STEPPED_DOWN", "Upstream's equality form",
                 "a MsgProp is dropped", "no RAFTQ_OUTF_ANSWERED", "does not end it", "`from` >= N is malformed",
                 "raftq_node does not turn the switch on"):
        assert said in rules, said
    assert "RAFTQ_OUT_CAMPAIGN / RAFTQ_OUT_BECAME_LEADER / RAFTQ_OUT_PRE_CAMPAIGN" in step_h  # the 40-byte record's paragraph
    assert "and so does a RAFTQ_OUT_PRE_CAMPAIGN" in step_h  # the 32-byte record's


def test_documents_name_it():
    design = _read("DESIGN.md")
    assert "raftq_set_pre_vote" in design and "profiles/r27" in design
    assert not re.search(r"PreVote and leadership transfer,? (which )?are not modelled", design)
    for doc in ("README.md", "INTEGRATION.md", os.path.join("go", "raftq", "README.md")):
        assert "raftq_set_pre_vote" in _read(doc), doc
    integration = _read("INTEGRATION.md")
    for name in ("RAFTQ_OUT_PRE_CAMPAIGN", "RAFTQ_OUT_PRE_VOTE_RESP", "RAFTQ_OUT_TERM_RESP"):
        assert name in integration, name
    assert os.path.exists(os.path.join(ROOT, "profiles", "r27", "README.md"))
    assert os.path.exists(os.path.join(ROOT, "tools", "profile_pre_vote.py"))
