"""defuse_amd/capi.py, the layer every ctypes binding shares, against a stand-in library that records its calls (no GPU and
no built library), and every header of include/ against the module that binds it."""
import ctypes
import importlib
import os
import re

import pytest

from defuse_amd import capi
from tests import abi


class FakeFunction:
    def __init__(self, log, name):
        self.log, self.name, self.restype, self.argtypes = log, name, ctypes.c_int, None

    def __call__(self, *args):
        self.log.append((self.name, [a.value if hasattr(a, "value") else a for a in args]))
        return 0


class FakeLibrary:
    """Has thing_destroy and thing_last_error, nothing else; .calls is the log."""

    def __init__(self):
        self.calls = []
        self.thing_destroy = FakeFunction(self.calls, "thing_destroy")
        self.thing_last_error = FakeFunction(self.calls, "thing_last_error")


class Thing(capi.Owned):
    _destroy = "thing_destroy"

    def __init__(self, lib, value=7, fail=None):
        if fail == "early":
            raise ValueError("before the base was set up")
        super().__init__(lib)
        if fail == "late":
            raise ValueError("before the handle was set")
        self.handle.value = value


def test_owned_destroys_exactly_once():
    lib = FakeLibrary()
    t = Thing(lib)
    assert isinstance(t.handle, ctypes.c_void_p) and t.handle.value == 7
    t.close()
    assert lib.calls == [("thing_destroy", [7])] and isinstance(t.handle, ctypes.c_void_p) and not t.handle
    t.close()                                       # the handle is null: a no-op
    del t
    assert lib.calls == [("thing_destroy", [7])]
    t = Thing(lib, 9)
    del t                                           # never closed: __del__ frees it
    assert lib.calls == [("thing_destroy", [7]), ("thing_destroy", [9])]


def test_owned_with_block_closes():
    lib = FakeLibrary()
    with Thing(lib, 3) as t:
        assert t.handle.value == 3 and lib.calls == []
    assert lib.calls == [("thing_destroy", [3])] and not t.handle
    with pytest.raises(KeyError):
        with Thing(lib, 4):
            raise KeyError("the block fails")
    assert lib.calls[-1] == ("thing_destroy", [4])


@pytest.mark.parametrize("fail", ["early", "late"])
def test_owned_del_is_silent_on_a_half_constructed_object(fail):
    lib = FakeLibrary()
    t = Thing.__new__(Thing)
    with pytest.raises(ValueError):
        t.__init__(lib, fail=fail)
    assert not t.handle
    t.close()
    t.__del__()
    assert lib.calls == []


def test_owned_del_never_raises():
    class Broken(Thing):
        _destroy = "no_such_function"
    b = Broken(FakeLibrary())
    with pytest.raises(AttributeError):
        b.close()
    b.__del__()                                     # as at interpreter shutdown, when the library may be gone


def test_bind_applies_a_table_once():
    lib = FakeLibrary()
    table = {"thing_destroy": (None, [ctypes.c_void_p]), "thing_last_error": (ctypes.c_char_p, [])}
    assert capi.bind(lib, table) is lib
    assert lib.thing_destroy.restype is None and lib.thing_destroy.argtypes == [ctypes.c_void_p]
    assert lib.thing_last_error.restype is ctypes.c_char_p and lib.thing_last_error.argtypes == []
    lib.thing_destroy.argtypes = "touched"
    assert capi.bind(lib, table) is lib and lib.thing_destroy.argtypes == "touched"           # the second call does nothing
    other = FakeLibrary()
    capi.bind(other, table)                                                                   # another library: bound afresh
    assert other.thing_destroy.argtypes == [ctypes.c_void_p]
    with pytest.raises(AttributeError):
        capi.bind(FakeLibrary(), {"thing_create": (ctypes.c_int, [])})


def test_errors_format_as_before():
    from defuse_amd import bat, cand, cmp, cov, dsa, pred, ptext, task, text
    assert str(pred.PredError(-3, "x")) == "pred error -3: x" and pred.PredError(-3, "x").code == -3
    assert str(dsa.DsaError(-1, "y")) == "dsa error -1: y" and dsa.DsaError(-1, "y").code == -1
    for cls, prefix in ((bat.BatError, "bat"), (cand.CandError, "cand"), (cmp.CmpError, "cmp"), (cov.CovError, "cov"), (ptext.PtextError, "ptext"),
                        (task.TaskError, "task"), (text.TextError, "text")):
        e = cls(-4, "z")
        assert str(e) == "%s error -4: z" % prefix and e.code == -4 and isinstance(e, capi.ApiError) and isinstance(e, RuntimeError)
    assert (capi.E_CAPACITY, capi.E_DEVICE, capi.E_ARG, capi.E_LIMIT, capi.E_BUSY) == (-1, -2, -3, -4, -5)
    assert (pred.DSA_E_ARG, cmp.DSA_E_CAPACITY, dsa.DSA_E_BUSY) == (-3, -1, -5)


def test_ptr_and_as_dict():
    import numpy as np

    class Timing(ctypes.Structure):
        _fields_ = [("a_ms", ctypes.c_float), ("pad_", ctypes.c_float), ("n", ctypes.c_int64)]
    assert capi.as_dict(Timing(1.5, 9.0, 4)) == {"a_ms": 1.5, "n": 4}
    a = np.arange(3)
    assert capi.ptr(a) == a.ctypes.data and capi.ptr(a[:0]) is None


# ---------------------------------------------------------------------------------------------- every header of include/
# (header, the regex of its functions' names, its binding module, the number of functions it declares)
HEADERS = [("defuse_bat.h", r"(?:bat|cand)_[a-z_]+", "bat", 14), ("defuse_cand.h", r"cand_[a-z_]+", "cand", 8), ("defuse_cmp.h", r"cmp_[a-z_]+", "cmp", 17),
           ("defuse_cov.h", r"cov_[a-z_]+", "cov", 2), ("defuse_dsa.h", r"dsa_[a-z_]+", "dsa", 35), ("defuse_est.h", r"est_[a-z_]+", "est", 5),
           ("defuse_eval.h", r"eval_\w+", "eval", 6), ("defuse_hc.h", r"hc_[a-z_]+", "hc", 2), ("defuse_la.h", r"la_[a-z_]+", "la", 6),
           ("defuse_mpe.h", r"mpe_[a-z_]+", "mpe", 4), ("defuse_pred.h", r"pred_[a-z_]+", "pred", 10), ("defuse_ptext.h", r"ptext_[a-z_]+", "ptext", 10),
           ("defuse_rec.h", r"rec_[a-z_]+", "rec", 14), ("defuse_sc.h", r"sc_[a-z_]+", "sc", 3), ("defuse_task.h", r"task_[a-z_]+", "task", 12),
           ("defuse_text.h", r"(?:txt|cand|bat)_[a-z_]+", "text", 17)]
ALL = [h[0] for h in HEADERS]
# what only one header may speak of, comments included: (header, pattern, the headers that must not have it)
APART = [("defuse_pred.h", r"pred_", ["defuse_eval.h", "defuse_bat.h", "defuse_cand.h"]),
         ("defuse_task.h", r"task_", ["defuse_eval.h", "defuse_bat.h", "defuse_cand.h", "defuse_pred.h"]),
         ("defuse_ptext.h", r"ptext_(?!shared)", ALL),
         ("defuse_text.h", r"\btxt_|cand_enumerate_resident|bat_reads_create_device", ALL)]


@pytest.mark.parametrize("header,prefix,module,count", HEADERS, ids=ALL)
def test_header_and_module_declare_the_same_functions(built, header, prefix, module, count):
    """tests/abi.py:check_functions for every header of include/, with the number of functions each declares; and what is
    one header's alone is in no other."""
    m = importlib.import_module("defuse_amd." + module)
    assert abi.check_functions(header, m, prefix) == count == len(m.EXPORTS) == len(m.PROTOTYPES)
    for owner, pattern, others in APART:
        if header in others and header != owner:
            assert not re.search(pattern, open(os.path.join(abi.INCLUDE, header)).read()), (header, pattern)


def test_every_header_is_in_the_table_and_every_function_in_one_module():
    assert sorted(os.listdir(abi.INCLUDE)) == sorted(ALL)
    names = [n for _, _, module, _ in HEADERS for n in importlib.import_module("defuse_amd." + module).PROTOTYPES]
    assert len(names) == len(set(names)) == sum(h[3] for h in HEADERS)
