"""CPU: the per-group voter-set entry points exist where a caller looks for them -- declared in include/raftq.h with their
16-byte record, exported by the library, bound by the package -- and refuse a NULL handle without touching a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("raftq_load_voters", "raftq_apply_voter_deltas", "raftq_read_voters")


@pytest.fixture(scope="module")
def lib():
    from raftsql_amd import _lib, build

    build.build_lib()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "raftq.h")).read(), flags=re.S)


def test_header_declares_the_three_calls_and_the_record():
    hdr = _header()
    assert re.search(r"int\s+raftq_load_voters\s*\(\s*raftq_t\s*\*\s*h\s*,\s*const\s+uint16_t\s*\*\s*voters\s*\)\s*;", hdr)
    assert re.search(r"int\s+raftq_apply_voter_deltas\s*\(\s*raftq_t\s*\*\s*h\s*,\s*const\s+raftq_voter_delta_t\s*\*\s*d\s*,\s*uint64_t\s+n\s*\)\s*;", hdr)
    assert re.search(r"int\s+raftq_read_voters\s*\(\s*raftq_t\s*\*\s*h\s*,\s*uint16_t\s*\*\s*voters_out\s*\)\s*;", hdr)
    m = re.search(r"typedef\s+struct\s+raftq_voter_delta\s*\{(.*?)\}\s*raftq_voter_delta_t\s*;", hdr, flags=re.S)
    assert m
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["uint64_t group", "uint16_t voters", "uint16_t reset", "uint32_t _pad"]


def test_the_record_is_16_bytes_for_a_c_compiler_and_for_the_binding(tmp_path):
    from raftsql_amd import _lib
    from raftsql_amd.engine import QuorumEngine

    src = tmp_path / "voter_delta_size.c"
    src.write_text('#include <stddef.h>\n#include "raftq.h"\n'
                   "typedef char size_is_16[sizeof(raftq_voter_delta_t) == 16 ? 1 : -1];\n"
                   "typedef char voters_at_8[offsetof(raftq_voter_delta_t, voters) == 8 ? 1 : -1];\n"
                   "typedef char reset_at_10[offsetof(raftq_voter_delta_t, reset) == 10 ? 1 : -1];\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    assert C.sizeof(_lib.VoterDelta) == 16 and _lib.VoterDelta.voters.offset == 8 and _lib.VoterDelta.reset.offset == 10
    dt = QuorumEngine._VOTER_DELTA_DT
    assert dt.itemsize == 16 and dt.fields["voters"][1] == 8 and dt.fields["reset"][1] == 10
    a = QuorumEngine.pack_voter_deltas([3, 9], [0b101, 0b11], [0, 0b10])
    assert a.tobytes() == (3).to_bytes(8, "little") + b"\x05\x00\x00\x00" + bytes(4) + (9).to_bytes(8, "little") + b"\x03\x00\x02\x00" + bytes(4)


def test_library_exports_and_package_binds_them(lib):
    from raftsql_amd import _lib

    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def test_null_handle_is_einval(lib):
    from raftsql_amd import _lib

    buf = (C.c_uint16 * 4)()
    rec = _lib.VoterDelta(0, 1, 0, 0)
    assert lib.raftq_load_voters(None, None) == _lib.RAFTQ_EINVAL
    assert lib.raftq_load_voters(None, C.addressof(buf)) == _lib.RAFTQ_EINVAL
    assert lib.raftq_apply_voter_deltas(None, C.addressof(rec), 1) == _lib.RAFTQ_EINVAL
    assert lib.raftq_apply_voter_deltas(None, None, 0) == _lib.RAFTQ_EINVAL
    assert lib.raftq_read_voters(None, C.addressof(buf)) == _lib.RAFTQ_EINVAL
    assert b"null handle" in lib.raftq_last_error(None)
