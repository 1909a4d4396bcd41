"""CPU: ReadIndex's three exports, its two message kinds, its two result kinds, its flag and its modes exist where a caller looks for
them -- declared in include/raftq.h and include/raftq_step.h, exported by the library, bound by the package and by the Go source --,
the calls validate a NULL handle without touching a device, no record changed size, the compact expanders read a sequence number out
of the commit slot, and the headers and documents state the contract."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFINES = {"RAFTQ_MSG_READ_INDEX": 15, "RAFTQ_MSG_READ_INDEX_RESP": 16, "RAFTQ_OUT_READ_INDEX": 18, "RAFTQ_OUT_READ_STATE": 19}
MODES = {"RAFTQ_READ_SAFE": 1, "RAFTQ_READ_LEASE": 2}
CALLS = ("raftq_set_read_index", "raftq_load_reads", "raftq_read_reads")


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
    assert re.search(r"int\s+raftq_set_read_index\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int\s+mode\s*\)\s*;", hdr)
    assert re.search(r"int\s+raftq_load_reads\s*\(\s*raftq_t\s*\*\s*h\s*,\s*const\s+uint32_t\s*\*\s*seq\s*,\s*const\s+uint32_t\s*\*\s*acked\s*\)\s*;", hdr)
    assert re.search(r"int\s+raftq_read_reads\s*\(\s*raftq_t\s*\*\s*h\s*,\s*uint32_t\s*\*\s*seq\s*,\s*uint32_t\s*\*\s*acked\s*,\s*uint32_t\s*\*\s*confirmed\s*\)\s*;", hdr)
    for name, value in MODES.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
    for name, value in DEFINES.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), step_h), name
    assert re.search(r"#define\s+RAFTQ_OUTF_READ_READY\s+\(1u\s*<<\s*6\)", step_h)  # = 0x40
    # the values that were there keep theirs, and the new flag takes a bit that was free
    for name, value in (("RAFTQ_MSG_TIMEOUT_NOW", 14), ("RAFTQ_MSG_PRE_VOTE", 17), ("RAFTQ_OUT_TRANSFER", 17), ("RAFTQ_OUT_TERM_RESP", 16)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), step_h), name
    flags = {n: int(v, 16) for n, v in re.findall(r"#define\s+(RAFTQ_OUTF_\w+)\s+0x([0-9a-fA-F]+)u", step_h + _code(_read("include", "raftq_wire.h")))}
    assert all(v & 0x40 == 0 for v in flags.values())


def test_the_constants_compile_to_their_values(tmp_path):
    """the preprocessor's own word on the flag and the modes (cc -E on a C file that includes the headers)"""
    import shutil
    import subprocess

    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None  # (the oracle is built with it)
    src = tmp_path / "v.c"
    src.write_text('#include "raftq.h"\n#include "raftq_step.h"\n'
                   "_Static_assert(RAFTQ_OUTF_READ_READY == 0x40u, \"flag\");\n_Static_assert(RAFTQ_READ_SAFE == 1 && RAFTQ_READ_LEASE == 2, \"modes\");\n"
                   "_Static_assert(RAFTQ_MSG_READ_INDEX == 15 && RAFTQ_MSG_READ_INDEX_RESP == 16 && RAFTQ_OUT_READ_INDEX == 18 && RAFTQ_OUT_READ_STATE == 19, \"kinds\");\n"
                   "_Static_assert(sizeof(raftq_msg_t) == 64 && sizeof(raftq_msg40_t) == 40 && sizeof(raftq_step_out_t) == 64 && sizeof(raftq_step_out_c_t) == 40 && "
                   "sizeof(raftq_step_out_s_t) == 32, \"sizes\");\nint main(void) { return 0; }\n")
    p = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


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
    for name in ("set_read_index", "load_reads", "read_reads"):
        assert callable(getattr(QuorumEngine, name, None)), name
    assert (_lib.READ_SAFE, _lib.READ_LEASE) == (1, 2)
    assert (step.MSG_READ_INDEX, step.MSG_READ_INDEX_RESP, step.OUT_READ_INDEX, step.OUT_READ_STATE, step.OUTF_READ_READY) == (15, 16, 18, 19, 0x40)
    assert step.MSG_READ_INDEX not in step.MSG_TYPES and step.MSG_READ_INDEX_RESP not in step.MSG_TYPES  # (the kinds every handle takes)
    from tests import ref_read_index as RI

    assert (RI.MsgReadIndex, RI.MsgReadIndexResp, RI.OutReadIndex, RI.OutReadState, RI.FlagReadReady, RI.SAFE, RI.LEASE) == (15, 16, 18, 19, 0x40, 1, 2)


def test_go_source_binds_them():
    go, step_go = _read("go", "raftq", "raftq.go"), _read("go", "raftq", "step.go")
    assert re.search(r"func \(e \*Engine\) SetReadIndex\(mode int\) error", go) and "C.raftq_set_read_index(e.h, v)" in go
    assert re.search(r"func \(e \*Engine\) LoadReads\(seq \[\]uint32, acked \[\]uint32\) error", go) and "C.raftq_load_reads(e.h, s, a)" in go
    assert re.search(r"func \(e \*Engine\) ReadReads\(seq \[\]uint32, acked \[\]uint32, confirmed \[\]uint32\) error", go) and "C.raftq_read_reads(e.h, s, a, c)" in go
    for name in MODES:
        assert "C." + name in go, name
    for name in list(DEFINES) + ["RAFTQ_OUTF_READ_READY"]:
        assert "C." + name in step_go, name
    readme = _read("go", "raftq", "README.md")
    for name in ("SetReadIndex", "LoadReads", "ReadReads", "MsgReadIndex", "MsgReadIndexResp", "OutReadIndex", "OutReadState", "FlagReadReady", "ReadSafe", "ReadLease"):
        assert name in readme, name
    assert "SetReadIndex" in _read("go", "raftq", "PIN.md")


def test_null_handle_touches_no_device(lib):
    from raftsql_amd import _lib

    for mode in (0, 1, 2, 3):
        assert lib.raftq_set_read_index(None, mode) == _lib.RAFTQ_EINVAL
    assert b"null handle" in lib.raftq_last_error(None)
    buf = (C.c_uint32 * 4)()
    p = C.cast(buf, C.c_void_p)
    assert lib.raftq_load_reads(None, p, p) == _lib.RAFTQ_EINVAL
    assert lib.raftq_read_reads(None, p, p, p) == _lib.RAFTQ_EINVAL
    assert bytes(buf) == b"\0" * 16 and b"null handle" in lib.raftq_last_error(None)


def test_the_compact_expanders_read_the_sequence_number_out_of_the_commit_slot():
    """raftsql_amd.step.expand_compact / expand_short: RAFTQ_OUT_READ_INDEX and a RAFTQ_OUT_PROGRESS with RAFTQ_OUTF_READ_READY carry
    log_term in the commit slot; the first one's commit IS its index, the second one's is the index that stood; RAFTQ_OUT_READ_STATE
    and a progress result without the flag pack as they always did"""
    from raftsql_amd import step

    m = step.pack_msgs([3, 3, 3, 3], step.MSG_HEARTBEAT_RESP, frm=2)
    c = np.zeros(4, step.OUT_C_DT)
    c["type"] = (step.OUT_READ_INDEX, step.OUT_PROGRESS, step.OUT_PROGRESS, step.OUT_READ_STATE)
    c["flags"] = (0, step.OUTF_READ_READY, 0, 0)
    c["term"], c["index"], c["commit"], c["aux"], c["role"] = 5, (6, 4, 4, 6), (9, 8, 6, 6), 7, 2
    o = step.expand_compact(m, c)
    assert o["log_term"].tolist() == [9, 8, 0, 0] and o["commit"].tolist() == [6, 0, 6, 6] and o["last_index"].tolist() == [7] * 4
    assert o["index"].tolist() == [6, 4, 4, 6] and o["to"].tolist() == [2] * 4 and o["flags"].tolist() == [0, step.OUTF_READ_READY, 0, 0]
    s = np.zeros(4, step.OUT_S_DT)
    for k in ("type", "flags", "term", "index", "commit", "role"):
        s[k] = c[k]
    o = step.expand_short(m, s, np.full(4, 7, np.uint64), np.full(4, 2, np.uint64))
    assert o["log_term"].tolist() == [9, 8, 0, 0] and o["commit"].tolist() == [6, 6, 6, 6] and o["last_index"].tolist() == [7] * 4


def test_headers_state_the_contract():
    raftq_h, step_h, wire_h = _flat("include", "raftq.h"), _flat("include", "raftq_step.h"), _flat("include", "raftq_wire.h")
    assert raftq_h.index("Leadership transfer: MsgTransferLeader") < raftq_h.index("ReadIndex: linearizable reads")  # behind "Leadership transfer"
    switch = raftq_h[raftq_h.index("ReadIndex: linearizable reads"):raftq_h.index("int raftq_read_reads")]
    for said in ("PARITY UNPINNED", "RAFTQ_READ_SAFE", "RAFTQ_READ_LEASE", "ReadOnlySafe", "ReadOnlyLeaseBased", "anything but 0, 1 or 2 is RAFTQ_EINVAL",
                 "no device is touched", "raftq_clone_state does not copy the switch", "Every change of mode zeroes the state", "mode 0 frees it",
                 "CHOICE", "check quorum", "read index", "Independent of raftq_set_pre_vote", "RAFTQ_READ_LEASE holds none", "one 64-byte record per group",
                 "no read traffic and no reset()", "one zeroed record", "confirmed(g) is not stored", "q_g = popcount / 2 + 1", "an empty mask gives 0",
                 "stored and does not count", "nothing is loaded", "copies the records when both handles hold them", "raftq_tick_frames",
                 "raftq_tick_elect_frames", "RAFTQ_READ_LEASE closes nothing", "raftq_node does not turn the switch on"):
        assert said in switch, said
    rules = step_h[step_h.index("ReadIndex in Step"):step_h.index("raftq_msg_t._pad[1] once the handle opted in")]
    for said in ("PARITY UNPINNED", "CHOICE", "unknown kinds that fail their batch", "REQUESTER's slot", "as for MsgProp", "malformed even at term 0",
                 "Entries[0].Data", "result i answers record i", "first_idx == 0 || committed < first_idx", "etcd 3.3 / 3.4", "seq == 2^32 - 1",
                 "to = from, index = committed", "log_term = 0 and RAFTQ_OUTF_READ_READY", "acked[self] = seq", "confirmed() >= seq already",
                 "bcastHeartbeatWithCtx", "only the last one's round needs sending", "this wire has no Context field", "c > seq", "max(acked[p], c)",
                 "after > before", "`index` stays Match", "counts for every request <= c", "never a later one", "loss, duplication and reordering",
                 "readOnly = newReadOnly", "RAFTQ_OUTF_STEPPED_DOWN", "does NOT clear it", "lastPendingRequestCtx", "RAFTQ_OUT_FORWARD, to = lead - 1",
                 "the echo", "a lease-mode follower may sit under a safe-mode leader", "RAFTQ_OUT_READ_STATE", "becomeFollower(m.Term, None)",
                 "`commit` slot of both the 40-byte and the 32-byte record", "commit IS its `index`", "moves no commit index", "Index = m.index",
                 "no RAFTQ_OUTF_ANSWERED", "stops no commit broadcast", "No encoder builds types 15 and 16 on the device",
                 "raftq_node does not turn the switch on"):
        assert said in rules, said
    for said in ("raftq_set_read_index", "types 15 and 16", "its context as an entry", "wide record in the packed form", "RAFTQ_OUT_READ_INDEX",
                 "RAFTQ_OUT_READ_STATE", "RAFTQ_OUTF_READ_READY", "No encoder builds the two kinds on the device"):
        assert said in wire_h, said


def test_documents_name_it():
    design = _read("DESIGN.md")
    assert "raftq_set_read_index" in design and "profiles/r30" in design
    for left in ("Device-built heartbeat rounds that carry the pending context", "MsgReadIndexResp frames built on the device",
                 "Queuing a read that arrives before the leader's first commit"):
        assert left in design, left
    for doc in ("README.md", "INTEGRATION.md", os.path.join("go", "raftq", "README.md")):
        assert "raftq_set_read_index" in _read(doc), doc
    integration = _read("INTEGRATION.md")
    for name in ("RAFTQ_MSG_READ_INDEX", "RAFTQ_OUT_READ_INDEX", "RAFTQ_OUTF_READ_READY", "RAFTQ_OUT_READ_STATE", "MsgReadIndexResp", "(seq, index, context, from)"):
        assert name in integration, name
    assert "test_read_index" in _read("README.md")
    assert os.path.exists(os.path.join(ROOT, "profiles", "r30", "README.md"))
