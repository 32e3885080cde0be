"""Replay of recorded C-ABI calls (test infrastructure only): the cases of
tests/golden/abi_errors.json, written by tests/golden/gen_abi_errors.py from the
library of the commit before the entry points were refactored. Every case
returns before the library's first HIP call, so no GPU is needed, and every
pointer is a small integer that is never dereferenced.

A case is {"fn", "args", "ret", "err"}. An argument is an integer (a count, a
size or a pointer value), null, or one of
  {"scene": {field: value}}  a ptmi_scene_view, zero but for these fields
  {"frame": {field: value}}  a ptmi_frame, zero (camera included) but for these
  {"f": "0.05"}              a C float
  {"i32p": 64}               an int32_t* of that value
``ret`` is the call's return value and ``err`` the text of ptmi_last_error()
after it. Before each call the error text is set to SENTINEL by a rejected
ptmi_prof_start, so a silent no-op shows as ret 0 with err == SENTINEL."""
import ctypes as C
import json
import os

from ptmi import _lib

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'abi_errors.json')
SENTINEL = 'max_launches < 0'


def _struct(cls, fields):
    s = cls()
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def _arg(a, keep):
    if not isinstance(a, dict):
        return a
    (kind, v), = a.items()
    if kind == 'f':
        return float(v)
    if kind == 'i32p':
        return C.cast(C.c_void_p(v), C.POINTER(C.c_int32)) if v else None
    s = _struct(_lib.SceneView if kind == 'scene' else _lib.Frame, v)
    keep.append(s)
    return C.byref(s)


def call(lib, fn, args):
    """(return value, last-error text) of one recorded call."""
    assert lib.ptmi_prof_start(-1) == _lib.PTMI_EINVAL
    keep = []
    ret = getattr(lib, fn)(*[_arg(a, keep) for a in args])
    return int(ret), lib.ptmi_last_error().decode()


def load_table():
    with open(TABLE) as f:
        return json.load(f)
