"""CPU: the decoder's narrow output forms (include/raftq_wire.h: raftq_wire_decode_packed, raftq_step_frames_packed) are
declared, bound and exported and refuse without a device; the two narrow records have the sizes and offsets the header
gives them; RAFTQ_WIRE_F_WIDE is a flag bit of its own; and the narrowing rule -- stated in tests/packed_rule.py from the
header text -- applied to the oracle's records and fed through raftsql_amd.wire.expand_packed gives the oracle's records
back.  No compute is called here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import packed_rule as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from raftsql_amd import _lib, build

    build.build_lib()
    return _lib.load()


def _text(*path):
    return open(os.path.join(ROOT, *path)).read()


def _define(text, name):
    m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)u?\b" % name, text)
    assert m, name
    return int(m.group(1), 0)


def test_the_calls_are_declared_bound_and_exported(lib):
    from raftsql_amd import _lib

    sigs = dict((s[0], s[2]) for s in _lib._WIRE_SIGS)
    hdr = re.sub(r"/\*.*?\*/", "", _text("include", "raftq_wire.h"), flags=re.S)
    for name in ("raftq_wire_decode_packed", "raftq_step_frames_packed"):
        assert name in _lib.WIRE_EXPORTS and hasattr(lib, name)
        proto = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr)
        assert proto and len(sigs[name]) == len(proto.group(1).split(",")) == 15, name


def test_refuse_without_a_handle(lib):
    from raftsql_amd import _lib

    wc, nw = _lib.WireCounts(), C.c_uint64(7)
    rc = lib.raftq_wire_decode_packed(None, None, 0, None, 0, 40, 0, 0, None, None, 0, None, 0, C.byref(wc), C.byref(nw))
    assert rc in (_lib.RAFTQ_EINVAL, _lib.RAFTQ_ENODEV)
    rc = lib.raftq_step_frames_packed(None, None, 0, None, 0, 1, 8, 0, None, None, 0, None, 0, C.byref(wc), C.byref(nw))
    assert rc in (_lib.RAFTQ_EINVAL, _lib.RAFTQ_ENODEV)


def test_record_sizes_and_offsets_are_msg40s():
    """raftq_wire_msg40_t is raftq_msg40_t's layout with the flags in its pad byte; raftq_wire_head_t is its first 8 bytes --
    in the header (natural alignment), the Python binding, the rule's own statement and the Go source"""
    from raftsql_amd import step as S
    from raftsql_amd import wire as W
    from tests.test_go_binding import c_structs, go_structs, layout

    cs = c_structs()
    m40, size40 = layout(cs["raftq_wire_msg40"])
    head, size_head = layout(cs["raftq_wire_head"])
    step40, step_size = layout(cs["raftq_msg40"])
    assert (size40, size_head, step_size) == (40, 8, 40)
    assert [(o, b) for _, o, b in m40] == [(o, b) for _, o, b in step40]
    assert [n for n, _, _ in m40] == ["group", "from", "type", "reject", "flags", "term", "index", "aux", "commit"]
    assert head == m40[:5]
    for dt in (W.WIRE_MSG40_DT, R.MSG40_DT):
        assert dt.itemsize == 40 and [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == m40
        assert [dt.fields[n][1] for n in dt.names] == [S.MSG40_DT.fields[n][1] for n in S.MSG40_DT.names]
    for dt in (W.WIRE_HEAD_DT, R.HEAD_DT):
        assert dt.itemsize == 8 and [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == head
    gs, _ = go_structs()
    g40, gsize40 = layout(gs["WireMsg40"])
    ghead, gsize_head = layout(gs["WireHead"])
    assert (gsize40, gsize_head) == (40, 8)
    assert [(n.lower(), o, b) for n, o, b in g40] == m40 and [(n.lower(), o, b) for n, o, b in ghead] == head


def test_wide_flag_is_a_bit_of_its_own():
    from raftsql_amd import step as S
    from raftsql_amd import wire as W

    h, step_h = _text("include", "raftq_wire.h"), _text("include", "raftq_step.h")
    wide = _define(h, "RAFTQ_WIRE_F_WIDE")
    assert wide == W.F_WIDE == R.F_WIDE == 0x08 and bin(wide).count("1") == 1
    wire_flags = [n for n in re.findall(r"#define\s+(RAFTQ_WIRE_F_\w+)", h) if n != "RAFTQ_WIRE_F_WIDE"]
    step_flags = re.findall(r"#define\s+(RAFTQ_MSGF_\w+)", step_h)
    assert len(wire_flags) == 3 and len(step_flags) >= 4
    for n in wire_flags:
        assert _define(h, n) & wide == 0, n
    for n in step_flags:
        assert _define(step_h, n) & wide == 0, n
    assert wide & (W.F_MALFORMED | W.F_SNAPSHOT | W.F_GROUP | S.MSGF_SKIP | S.MSGF_HOLD | S.MSGF_BARRIER | S.MSGF_ENTRIES) == 0
    assert (_define(h, "RAFTQ_WIRE_FORM_40"), _define(h, "RAFTQ_WIRE_FORM_HEAD")) == (W.FORM_40, W.FORM_HEAD) == (40, 8)
    go = _text("go", "raftq", "wire.go")
    assert re.search(r"WireWide\s*=\s*0x08\b", go) and re.search(r"WireForm40\s*=\s*40\b", go) and re.search(r"WireFormHead\s*=\s*8\b", go)
    for name in ("DecodePacked", "StepFramesPacked"):
        assert re.search(r"^func \(e \*Engine\) %s\(" % name, go, flags=re.M), name
    pin = _text("go", "raftq", "etcd_pin_test.go")
    for name in ("WireMsg40", "WireHead", "DecodePacked", "WireWide", "WireForm40", "WireFormHead"):
        assert name in pin, name


# ---- the rule, on the CPU alone -------------------------------------------------------------------------------------------
CORPORA = [("random", 21, 700, 0), ("noncanonical", 22, 0, 0), ("malformed", 0, 0, R.MALFORMED_TO_SLOT), ("fuzz", 23, 0, 0), ("node", 24, 513, 0)]


def _same(a, b, what):
    assert len(a) == len(b), what
    if a.tobytes() != b.tobytes():
        for i in range(len(a)):
            assert a[i].tobytes() == b[i].tobytes(), (what, i, a[i], b[i])


@pytest.mark.parametrize("form", [R.FORM_40, R.FORM_HEAD])
@pytest.mark.parametrize("kind,seed,n,to_slot", CORPORA)
def test_rule_then_expansion_gives_the_oracles_records_back(oracle, kind, seed, n, to_slot, form):
    from raftsql_amd import wire as W

    _, _, m, _, _ = R.oracle_decode(kind, seed, n)
    head_types = R.RESPONSE_KINDS if form == R.FORM_HEAD else 0
    narrow, wide = R.pack(m, to_slot, form, head_types)
    assert narrow.dtype.itemsize == form and len(narrow) == len(m)
    is_narrow = R.is_narrow(m, to_slot, form, head_types)
    assert np.array_equal((narrow["flags"] & R.F_WIDE) == 0, is_narrow) and len(wide) == int((~is_narrow).sum())
    back = W.expand_packed(narrow.view(W._FORM_DT[form]), wide.view(W.WIRE_MSG_DT), to_slot, form)
    _same(back, R.delivered(m, to_slot, form, head_types).view(W.WIRE_MSG_DT), f"{kind}, form {form}")
    assert not np.any(back["flags"] & R.F_WIDE)  # the bit exists only in the narrow record
    # a malformed frame is the all-zero record plus its flag, and always narrow -- whatever to_slot is
    bad = (m["flags"] & 1) != 0
    assert np.all(is_narrow[bad]) and np.all(R.is_narrow(m, 200, form, head_types)[bad])


def test_corpora_are_what_the_tests_need_them_to_be(oracle):
    """the node-shaped corpus yields both kinds of frame in either form; random_msgs almost only wide ones; the malformed and
    fuzz corpora do hold malformed frames; the acks-only corpus no wide frame in the lossless form"""
    _, _, m, e, bad = R.oracle_decode("node", 24, 513)
    assert bad == 0 and len(e) > 0 and set(m["type"]) == {3, 4, 5, 6, 8, 9} and np.all(m["to"] == 0)
    assert 0.10 < float((m["type"] == 3).mean()) < 0.20 and set(m["n_ents"][m["type"] == 3]) == {1, 2, 3}
    for form, lo, hi in ((R.FORM_40, 0.10, 0.20), (R.FORM_HEAD, 0.25, 0.60)):
        wide = ~R.is_narrow(m, 0, form, R.RESPONSE_KINDS)
        assert lo < float(wide.mean()) < hi, (form, float(wide.mean()))
    _, _, m, _, _ = R.oracle_decode("random", 21, 700)
    for form in (R.FORM_40, R.FORM_HEAD):
        narrow = R.is_narrow(m, 0, form, R.RESPONSE_KINDS)
        assert float(narrow.mean()) < 0.05, (form, float(narrow.mean()))
    assert R.oracle_decode("malformed")[4] == 10 and R.oracle_decode("fuzz", 23)[4] > 20
    _, _, m, e, _ = R.oracle_decode("acks", 25, 513)
    assert len(e) == 0 and np.all(R.is_narrow(m, 0, R.FORM_40)) and np.all(R.is_narrow(m, 0, R.FORM_HEAD, 0xFFFFFFFF))
    assert not np.any(R.is_narrow(m, 1, R.FORM_40))  # read as another slot's: every frame wide


def test_expansion_refuses_an_inconsistent_pair(oracle):
    from raftsql_amd import wire as W

    _, _, m, _, _ = R.oracle_decode("node", 24, 513)
    narrow, wide = R.pack(m, 0, R.FORM_40)
    with pytest.raises(AssertionError):  # wide[] shorter than the narrow array says (a wide_cap that was too small)
        W.expand_packed(narrow.view(W.WIRE_MSG40_DT), wide[:-1].view(W.WIRE_MSG_DT), 0, R.FORM_40)
    twisted = narrow.copy()
    k = np.nonzero(twisted["flags"] & R.F_WIDE)[0][3]
    twisted["aux"][k] += 1
    with pytest.raises(AssertionError):  # aux of a wide frame is not its position
        W.expand_packed(twisted.view(W.WIRE_MSG40_DT), wide.view(W.WIRE_MSG_DT), 0, R.FORM_40)
