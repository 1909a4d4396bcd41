"""CPU: the narrow mirror's two entry points exist where a caller looks for them -- declared in include/raftq.h, exported by
the library, bound by the package and by the Go source -- and refuse a NULL handle without touching a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("raftq_narrow", "raftq_narrow_rebuild")


@pytest.fixture(scope="module")
def lib():
    from raftsql_amd import _lib, build

    build.build_lib()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "raftq.h")).read(), flags=re.S)


def test_header_declares_the_two_calls():
    hdr = _header()
    assert re.search(r"int\s+raftq_narrow\s*\(\s*raftq_t\s*\*\s*h\s*,\s*int32_t\s*\*\s*valid_out\s*\)\s*;", hdr)
    assert re.search(r"int\s+raftq_narrow_rebuild\s*\(\s*raftq_t\s*\*\s*h\s*\)\s*;", hdr)


def test_header_is_c99(tmp_path):
    src = tmp_path / "narrow_decl.c"
    src.write_text('#include "raftq.h"\n'
                   "int (*const p_narrow)(raftq_t*, int32_t*) = raftq_narrow;\n"
                   "int (*const p_rebuild)(raftq_t*) = raftq_narrow_rebuild;\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_library_exports_and_package_binds_them(lib):
    from raftsql_amd import _lib
    from raftsql_amd.engine import QuorumEngine

    sigs = {s[0]: s for s in _lib._SIGS}
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert sigs["raftq_narrow"][1] is C.c_int and sigs["raftq_narrow"][2] == [C.c_void_p, C.POINTER(C.c_int32)]
    assert sigs["raftq_narrow_rebuild"][1] is C.c_int and sigs["raftq_narrow_rebuild"][2] == [C.c_void_p]
    assert callable(QuorumEngine.narrow) and callable(QuorumEngine.narrow_rebuild)


def test_go_source_binds_them():
    go = "".join(open(os.path.join(ROOT, "go", "raftq", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "go", "raftq"))) if f.endswith(".go"))
    assert re.search(r"C\.raftq_narrow\(e\.h, &\w+\)", go) and "C.raftq_narrow_rebuild(e.h)" in go


def test_null_handle_is_einval(lib):
    from raftsql_amd import _lib

    v = C.c_int32(7)
    assert lib.raftq_narrow(None, C.byref(v)) == _lib.RAFTQ_EINVAL
    assert lib.raftq_narrow(None, None) == _lib.RAFTQ_EINVAL
    assert lib.raftq_narrow_rebuild(None) == _lib.RAFTQ_EINVAL
    assert b"null handle" in lib.raftq_last_error(None)
    assert v.value == 7
