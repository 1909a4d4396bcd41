"""CPU: leadership transfer's three exports, its two message kinds, its result kind and its flag exist where a caller looks for them --
declared in include/raftq.h and include/raftq_step.h, exported by the library, bound by the package and by the Go source --, the calls
validate a NULL handle without touching a device, no record changed size, and the headers and documents state the contract."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFINES = {"RAFTQ_MSG_TRANSFER_LEADER": 13, "RAFTQ_MSG_TIMEOUT_NOW": 14, "RAFTQ_OUT_TRANSFER": 17}
CALLS = ("raftq_set_lead_transfer", "raftq_load_transfer", "raftq_read_transfer")


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


def test_headers_declare_the_calls_and_the_constants():
    hdr, step_h = _code(_read("include", "raftq.h")), _code(_read("include", "raftq_step.h"))
    assert re.search(r"int\s+raftq_set_lead_transfer\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert re.search(r"int\s+raftq_load_transfer\s*\(\s*raftq_t\s*\*\s*h\s*,\s*const\s+uint8_t\s*\*\s*transferee\s*\)\s*;", hdr)
    assert re.search(r"int\s+raftq_read_transfer\s*\(\s*raftq_t\s*\*\s*h\s*,\s*uint8_t\s*\*\s*transferee\s*\)\s*;", hdr)
    for name, value in DEFINES.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), step_h), name
    assert re.search(r"#define\s+RAFTQ_OUTF_TIMEOUT_NOW\s+0x20u", step_h)
    # the values that were there keep theirs, and the new flag is the one bit that was free
    for name, value in (("RAFTQ_MSG_CHECK_QUORUM", 12), ("RAFTQ_MSG_PRE_VOTE", 17), ("RAFTQ_OUT_TERM_RESP", 16), ("RAFTQ_OUT_FORWARD", 13)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), step_h), name
    flags = {n: int(v, 16) for n, v in re.findall(r"#define\s+(RAFTQ_OUTF_\w+)\s+0x([0-9a-fA-F]+)u", step_h + _code(_read("include", "raftq_wire.h")))}
    assert len(set(flags.values())) == len(flags) and flags["RAFTQ_OUTF_ANSWERED"] == 0x10 and sum(flags.values()) == 0x3F


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

    for name in CALLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    for name in ("set_lead_transfer", "load_transfer", "read_transfer"):
        assert callable(getattr(QuorumEngine, name, None)), name
    assert (step.MSG_TRANSFER_LEADER, step.MSG_TIMEOUT_NOW, step.OUT_TRANSFER, step.OUTF_TIMEOUT_NOW) == (13, 14, 17, 0x20)
    assert step.MSG_TRANSFER_LEADER not in step.MSG_TYPES and step.MSG_TIMEOUT_NOW not in step.MSG_TYPES  # (the kinds every handle takes)


def test_go_source_binds_them():
    go, step_go = _read("go", "raftq", "raftq.go"), _read("go", "raftq", "step.go")
    assert re.search(r"func \(e \*Engine\) SetLeadTransfer\(on bool\) error", go) and "C.raftq_set_lead_transfer(e.h, v)" in go
    assert re.search(r"func \(e \*Engine\) LoadTransfer\(transferee \[\]uint8\) error", go) and "C.raftq_load_transfer(e.h," in go
    assert re.search(r"func \(e \*Engine\) ReadTransfer\(transferee \[\]uint8\) error", go) and "C.raftq_read_transfer(e.h," in go
    for name in list(DEFINES) + ["RAFTQ_OUTF_TIMEOUT_NOW"]:
        assert "C." + name in step_go, name
    readme = _read("go", "raftq", "README.md")
    for name in ("SetLeadTransfer", "LoadTransfer", "ReadTransfer", "MsgTransferLeader", "MsgTimeoutNow", "OutTransfer", "FlagTimeoutNow"):
        assert name in readme, name


def test_null_handle_touches_no_device(lib):
    from raftsql_amd import _lib

    for on in (0, 1, 2):
        assert lib.raftq_set_lead_transfer(None, on) == _lib.RAFTQ_EINVAL
    assert b"null handle" in lib.raftq_last_error(None)
    import ctypes as C

    buf = (C.c_uint8 * 4)()
    assert lib.raftq_load_transfer(None, C.cast(buf, C.c_void_p)) == _lib.RAFTQ_EINVAL
    assert lib.raftq_read_transfer(None, C.cast(buf, C.c_void_p)) == _lib.RAFTQ_EINVAL
    assert bytes(buf) == b"\0\0\0\0" and b"null handle" in lib.raftq_last_error(None)


def test_the_compact_expanders_pack_a_transfer_as_progress():
    """raftsql_amd.step.expand_compact / expand_short recover a RAFTQ_OUT_TRANSFER as they recover a RAFTQ_OUT_PROGRESS; reject and the
    new flag ride as they are"""
    import numpy as np

    from raftsql_amd import step

    m = step.pack_msgs([3], step.MSG_TRANSFER_LEADER, frm=2)
    for typ, reject in ((step.OUT_TRANSFER, 0), (step.OUT_PROGRESS, 0), (step.OUT_CAMPAIGN, 1)):
        c = np.zeros(1, step.OUT_C_DT)
        c["term"], c["index"], c["commit"], c["aux"], c["type"], c["role"], c["flags"], c["reject"] = 5, 4, 2, 7, typ, 2, step.OUTF_TIMEOUT_NOW, reject
        o = step.expand_compact(m, c)[0]
        tip = typ == step.OUT_CAMPAIGN
        assert (int(o["log_term"]), int(o["last_index"]), int(o["index"]), int(o["to"])) == ((7, 4, 4, 2) if tip else (0, 7, 4, 2)), typ
        assert (int(o["flags"]), int(o["reject"])) == (step.OUTF_TIMEOUT_NOW, reject)
    s = np.zeros(1, step.OUT_S_DT)
    s["term"], s["index"], s["commit"], s["type"], s["role"], s["flags"] = 5, 4, 2, step.OUT_TRANSFER, 2, step.OUTF_TIMEOUT_NOW
    o = step.expand_short(m, s, np.full(4, 7, np.uint64), np.full(4, 2, np.uint64))[0]
    assert (int(o["log_term"]), int(o["last_index"]), int(o["commit"]), int(o["index"]), int(o["flags"])) == (0, 7, 2, 4, step.OUTF_TIMEOUT_NOW)


def test_headers_state_the_contract():
    raftq_h, step_h, wire_h = _flat("include", "raftq.h"), _flat("include", "raftq_step.h"), _flat("include", "raftq_wire.h")
    switch = raftq_h[raftq_h.index("Leadership transfer: MsgTransferLeader"):raftq_h.index("int raftq_read_transfer")]
    for said in ("PARITY UNPINNED", "CHOICE: it requires CheckQuorum", "check quorum", "lead transfer", "independent of raftq_set_pre_vote",
                 "raftq_clone_state does not copy it", "bits 12..15", "NO TICK KERNEL CHANGES", "abortLeaderTransfer()", "raftq_read_activity never shows",
                 "keeps them as they are", "clears them in every group", "a value above n_peers is RAFTQ_EINVAL", "the transferee travels with it",
                 "raftq_propose_frames", "raftq_apply_log_deltas stays the caller's responsibility", "does not abort the transfer",
                 "raftq_node does not turn the switch on", "no device is touched"):
        assert said in switch, said
    rules = step_h[step_h.index("Leadership transfer in Step"):step_h.index("raftq_msg_t._pad[1] once the handle opted in")]
    for said in ("PARITY UNPINNED", "CHOICE", "unknown kinds that fail their batch", "`reject` byte is not looked at", "TRANSFEREE's slot",
                 "malformed even at term 0", "reject = 1", "CampaignTransfer", "only if reject == 0", "becomeFollower(m.Term, None)",
                 "A MsgPreVote is never marked", "pr == nil", "aborted first", "cancels a pending one", "lead_elapsed = 0", "index = Match[t]",
                 "Match[t] == last_index", "sendAppend(t)", "RAFTQ_OUTF_UPDATED", "inside the update branch", "ErrProposalDropped",
                 "whether or not the check passes", "RAFTQ_OUT_FORWARD, to = lead - 1", "NOT one of the kinds answered RAFTQ_OUT_TERM_RESP",
                 "promotable()", "no pre-candidate step", "RAFTQ_OUT_BECAME_LEADER", "packs as RAFTQ_OUT_PROGRESS does", "no RAFTQ_OUTF_ANSWERED",
                 "always the host's to send", "No encoder builds the two kinds on the device", "no Tick kernel changes",
                 "raftq_node does not turn the switch on"):
        assert said in rules, said
    for said in ("raftq_set_lead_transfer", "types 13 and 14", "RAFTQ_OUT_TRANSFER", "RAFTQ_OUTF_TIMEOUT_NOW"):
        assert said in wire_h, said


def test_documents_name_it():
    design = _read("DESIGN.md")
    assert "raftq_set_lead_transfer" in design and "profiles/r29" in design
    assert "Leadership transfer is not modelled anywhere" not in design
    for doc in ("README.md", "INTEGRATION.md", os.path.join("go", "raftq", "README.md")):
        assert "raftq_set_lead_transfer" in _read(doc), doc
    integration = _read("INTEGRATION.md")
    for name in ("TransferLeadership", "RAFTQ_MSG_TRANSFER_LEADER", "RAFTQ_OUT_TRANSFER", "RAFTQ_OUTF_TIMEOUT_NOW"):
        assert name in integration, name
    assert os.path.exists(os.path.join(ROOT, "profiles", "r29", "README.md"))
