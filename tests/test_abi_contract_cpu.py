"""CPU (no GPU): what the dispatcher (csrc/mhx_abi.cpp) answers when every argument of an entry point is zero -- NULL pointers,
0 integers, 0.0 doubles -- is the record of tests/golden/abi_null_contract.json (tools/record_abi_null_contract.py; taken from the
hand-written dispatcher before the typed forwarder replaced it): return value and mhx_last_error() text, compared exactly, for
every entry point mhx_abi.cpp defines except mhx_version and mhx_last_error.  Each of these calls ends in the entry's guard."""
import ctypes as C
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_null_contract.json")))
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "double": C.c_double}


@pytest.fixture(scope="module")
def raw(mhx):
    """the library through a binding of its own, so that the argtypes set here do not replace those of mhx/_lib.py"""
    lib = C.CDLL(mhx.LIB_PATH)
    lib.mhx_last_error.restype = C.c_char_p
    lib.mhx_ctx_create.argtypes = [C.c_int, C.c_int, C.c_void_p]
    return lib


def test_the_record_covers_every_entry_point_of_the_dispatcher():
    src = open(os.path.join(ROOT, "advancedmh.jl_amd", "csrc", "mhx_abi.cpp")).read()
    defined = set(re.findall(r'^extern "C" [\w ]+?[ *]+(mhx_\w+)\(', src, flags=re.M))
    recorded = [e["name"] for e in RECORD["entries"]]
    assert len(recorded) == len(set(recorded)) == 73
    assert set(recorded) == defined - {"mhx_version", "mhx_last_error"}


@pytest.mark.parametrize("entry", RECORD["entries"], ids=lambda e: e["name"])
def test_all_zero_arguments_answer_as_recorded(raw, entry):
    # a known failure first: an entry that sets no message leaves this one standing, and the record says so
    assert raw.mhx_ctx_create(0, 0, None) == -1 and raw.mhx_last_error().decode() == RECORD["sentinel"]
    fn = getattr(raw, entry["name"])
    fn.restype = C.c_char_p if entry["returns"] == "string" else C.c_int
    fn.argtypes = [C.c_void_p if k == "ptr" else SCALARS[k] for k in entry["args"]]
    value = fn(*[None if k == "ptr" else 0 for k in entry["args"]])
    if entry["returns"] == "string":
        value = value.decode()
    assert value == entry["value"]
    assert raw.mhx_last_error().decode() == entry["last_error"]
