"""CPU: the tally mirror's two entry points exist where a caller looks for them -- declared in include/raftq.h, exported by
the library, bound by the package and by the Go source -- and refuse a NULL handle without touching a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("raftq_tally", "raftq_tally_rebuild")


@pytest.fixture(scope="module")
def lib():
    from raftsql_amd import _lib, build

    build.build_lib()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "raftq.h")).read(), flags=re.S)


def test_header_declares_the_two_calls():
    hdr = _header()
    for name in NAMES:
        assert re.search(r"int\s+%s\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int32_t\s*\*\s*valid_out\s*\)\s*;" % name, hdr), name


def test_header_is_c99(tmp_path):
    src = tmp_path / "tally_decl.c"
    src.write_text('#include "raftq.h"\n'
                   "int (*const p_tally)(raftq_t*, int32_t*) = raftq_tally;\n"
                   "int (*const p_rebuild)(raftq_t*, int32_t*) = raftq_tally_rebuild;\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_library_exports_and_package_binds_them(lib):
    from raftsql_amd import _lib
    from raftsql_amd.engine import QuorumEngine

    sigs = {s[0]: s for s in _lib._SIGS}
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert sigs[name][1] is C.c_int and sigs[name][2] == [C.c_void_p, C.POINTER(C.c_int32)]
    assert callable(QuorumEngine.tally) and callable(QuorumEngine.tally_rebuild)


def test_go_source_binds_them():
    go = "".join(open(os.path.join(ROOT, "go", "raftq", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "go", "raftq"))) if f.endswith(".go"))
    assert re.search(r"C\.raftq_tally\(e\.h, &\w+\)", go) and re.search(r"C\.raftq_tally_rebuild\(e\.h, &\w+\)", go)


def test_null_handle_is_einval(lib):
    from raftsql_amd import _lib

    v = C.c_int32(7)
    for name in NAMES:
        assert getattr(lib, name)(None, C.byref(v)) == _lib.RAFTQ_EINVAL
        assert getattr(lib, name)(None, None) == _lib.RAFTQ_EINVAL
    assert b"null handle" in lib.raftq_last_error(None)
    assert v.value == 7
