#!/usr/bin/env python3
"""Record what every entry point of csrc/mhx_abi.cpp answers when all its arguments are zero (NULL pointers, 0 integers, 0.0
doubles): return value and mhx_last_error() text -> tests/golden/abi_null_contract.json, which tests/test_abi_contract_cpu.py
replays against the built library.  No GPU is needed: every such call ends in the dispatcher's guard.

The entries are the prototypes of include/mhx.h that mhx_abi.cpp defines: all but mhx_comm_*, mhx_group_*, mhx_compact_expand (their
own files) and mhx_version / mhx_last_error (no argument, no guard).  Before each call a known failure plants SENTINEL as the last
error, so an entry that sets no message records the sentinel.

    python3 tools/record_abi_null_contract.py [path/to/libmhx.so]
"""
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "double": C.c_double}
SENTINEL = "mhx_ctx_create: out is NULL"
# differences from the commit the record was first taken at (the hand-written dispatcher), kept when the record is taken again
NOTES = {"mhx_ctx_dtype": "the hand-written dispatcher returned MHX_EINVAL here without setting a message (the sentinel stayed)"}


def prototypes():
    """[(name, returns a string, [parameter kind])] in header order; a kind is a key of SCALARS or "ptr" """
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mhx.h")).read(), flags=re.S)
    out = []
    for ret, name, args in re.findall(r"^\s*([\w ]+?[\s*]+)(mhx_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S | re.M):
        args = " ".join(args.split())
        kinds = []
        for a in ([] if args in ("", "void") else args.split(",")):
            kinds.append("ptr" if "*" in a else [k for k in a.split() if k in SCALARS][0])
        out.append((name, "char" in ret, kinds))
    return out


def dispatcher_entries():
    skip = re.compile(r"mhx_(comm_|group_|compact_expand$|version$|last_error$)")
    return [p for p in prototypes() if not skip.match(p[0])]


def call_with_zeros(lib, name, is_str, kinds):
    """(return value, last error) of one entry with all-zero arguments; SENTINEL is the last error going in"""
    lib.mhx_last_error.restype = C.c_char_p
    lib.mhx_ctx_create.argtypes = [C.c_int, C.c_int, C.c_void_p]
    assert lib.mhx_ctx_create(0, 0, None) == -1 and lib.mhx_last_error().decode() == SENTINEL
    fn = getattr(lib, name)
    fn.restype = C.c_char_p if is_str else C.c_int
    fn.argtypes = [C.c_void_p if k == "ptr" else SCALARS[k] for k in kinds]
    rv = fn(*[None if k == "ptr" else 0 for k in kinds])
    return (rv.decode() if is_str else rv), lib.mhx_last_error().decode()


def main():
    lib = C.CDLL(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "advancedmh.jl_amd", "libmhx.so"))
    rec = []
    for name, is_str, kinds in dispatcher_entries():
        rv, msg = call_with_zeros(lib, name, is_str, kinds)
        e = {"name": name, "args": kinds, "returns": "string" if is_str else "int", "value": rv, "last_error": msg}
        if name in NOTES:
            e["note"] = NOTES[name]
        rec.append(e)
    path = os.path.join(ROOT, "tests", "golden", "abi_null_contract.json")
    with open(path, "w") as f:
        json.dump({"sentinel": SENTINEL, "entries": rec}, f, indent=1)
        f.write("\n")
    print("%d entries -> %s" % (len(rec), path))


if __name__ == "__main__":
    main()
