"""CPU tests of the device constant path (include/de_hip.h de_program_set_consts_device): the three symbols are
exported and declared, their null-argument answers, and the argument checks of ``Population.set_constants`` that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("de_program_set_consts_device", "de_program_get_consts", "de_program_consts_device_path")


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    _api.library()
    return _api


def test_library_exports_and_header_declares_the_three_symbols(api):
    lib = api.library()
    with open(os.path.join(ROOT, "include", "de_hip.h")) as fh:
        header = fh.read()
    for name in SYMBOLS:
        assert name in api.EXPORTS
        assert hasattr(lib, name), f"libde_hip.so lacks {name}"
        assert re.search(r"^int %s\(" % name, header, re.M), f"include/de_hip.h does not declare {name}"
    assert lib.de_abi_version() == 3  # additions only: the ABI version stays


def test_null_program_answers(api):
    lib = api.library()
    buf = (C.c_float * 4)()
    invalid = 1  # DE_ERR_INVALID_ARG
    assert lib.de_status_string(invalid).decode().upper().find("INVALID") >= 0
    assert lib.de_program_set_consts_device(None, C.cast(buf, C.c_void_p)) == invalid
    assert lib.de_program_set_consts_device(None, None) == invalid
    assert lib.de_program_get_consts(None, C.cast(buf, C.c_void_p)) == invalid
    assert lib.de_program_consts_device_path(None) == -1


def _shell(api, dtype, n_consts):
    """A Population that owns no program: enough for the checks that run before the library is called."""
    pop = object.__new__(api.Population)
    pop._h = None
    pop._occ = None
    pop.dtype = np.dtype(dtype)
    pop.n_consts = np.asarray(n_consts, dtype=np.int64)
    pop._slots_per_tree = pop.n_consts.copy()
    return pop


def test_set_constants_checks_dtype_size_and_residence_before_any_call(api):
    torch = pytest.importorskip("torch")
    pop = _shell(api, np.float32, [2, 0, 3])
    with pytest.raises(ValueError, match="float64"):
        pop.set_constants(torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError, match="wrong number of constants"):
        pop.set_constants(torch.zeros(4, dtype=torch.float32))
    with pytest.raises(ValueError, match="device"):  # a host tensor: numpy is the host route
        pop.set_constants(torch.zeros(5, dtype=torch.float32))
    with pytest.raises(ValueError, match="wrong number of constants"):
        pop.set_constants(np.zeros(6, dtype=np.float32))
    pop64 = _shell(api, np.float64, [1])
    with pytest.raises(ValueError, match="float32"):
        pop64.set_constants(torch.zeros(1, dtype=torch.float32))


def test_occurrence_index_fans_out_and_back(api):
    """GraphNode fan-out tables: one value per unique constant -> one per occurrence slot, and the first slot of every unique one."""
    pop = _shell(api, np.float32, [2, 1, 0, 3])
    pop._occ = [np.array([0, 1, 0]), None, None, np.array([2, 0, 1, 2, 2])]
    pop._slots_per_tree = np.array([3, 1, 0, 5], dtype=np.int64)
    idx = pop._occ_index()
    assert idx["fan"].tolist() == [0, 1, 0, 2, 5, 3, 4, 5, 5]
    assert idx["first"].tolist() == [0, 1, 3, 5, 6, 4]
    vals = np.arange(10.0, 16.0)
    assert np.array_equal(vals[idx["fan"]][idx["first"]], vals)
