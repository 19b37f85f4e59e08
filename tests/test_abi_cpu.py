"""CPU-side checks of the C-ABI library: it exists, loads, exports every symbol the two headers declare (the product
ABI include/rvcx.h, the kernel-level test entries include/rvcx_test.h), binds each with as many parameters as its
prototype has, and keeps the two surfaces apart (no compute calls: there is no GPU here)."""
import os
import re
import shutil
import subprocess

import pytest

from abi_headers import header_prototypes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the kernel-level entries that used to sit in rvcx.h: test-only, so declared in rvcx_test.h alone
MOVED_TO_TEST_HEADER = ["rvcx_set_conv_math", "rvcx_conv1d", "rvcx_conv1d_gen", "rvcx_conv1d_ex", "rvcx_conv2d3x3",
                        "rvcx_convtranspose2d_s2", "rvcx_flash_attention", "rvcx_resblock_pair"]


def header_symbols():
    return sorted(header_prototypes("rvcx.h"))


def test_header_lists_entry_points():
    syms = header_symbols()
    assert "rvcx_synth_infer" in syms and "rvcx_rmvpe" in syms and "rvcx_hubert" in syms
    assert len(syms) >= 12


def test_library_exports_every_header_symbol():
    from rvcx import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    product, test = set(header_prototypes("rvcx.h")), set(header_prototypes("rvcx_test.h"))
    exported = set(_lib.exported_symbols())
    missing = sorted((product | test) - exported)
    assert not missing, missing
    assert set(_lib.EXPORTS) == product
    assert set(_lib.TEST_EXPORTS) == test
    assert not product & test, sorted(product & test)
    assert len(_lib.EXPORTS) == len(product) and len(_lib.TEST_EXPORTS) == len(test)  # each symbol listed once


def test_bindings_take_as_many_parameters_as_the_prototypes():
    """For every entry point of both headers: the parameter count of the declaration equals len(argtypes) of its
    ctypes binding, in the table and on the loaded library."""
    from rvcx import _lib

    lib = _lib.load()
    protos = {**header_prototypes("rvcx.h"), **header_prototypes("rvcx_test.h")}
    table = {**_lib.SIG, **_lib.TEST_SIG}
    assert len(protos) >= 87
    wrong = {n: (k, len(table[n][1])) for n, k in protos.items() if len(table[n][1]) != k}
    assert not wrong, f"(prototype, binding) parameter counts differ: {wrong}"
    unbound = [n for n in protos if getattr(lib, n).argtypes is None or len(getattr(lib, n).argtypes) != protos[n]]
    assert not unbound, unbound


@pytest.mark.parametrize("header", ["rvcx.h", "rvcx_test.h"])
def test_header_compiles_alone_as_c99(header, tmp_path):
    """Each header is a C header a product can include on its own (rvcx_test.h includes rvcx.h itself)."""
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler (cc / gcc) on PATH")
    src = tmp_path / "one.c"
    src.write_text(f'#include "{header}"\n')
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-fsyntax-only",
                        "-I" + os.path.join(REPO, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr


def test_kernel_test_entries_are_declared_in_the_test_header_only():
    """The product header holds no entry that exists for the numerics tests, and the shim
    rvcx_set_generator_precision (an unconditional error since the per-hop rvcx_rt_opts.gen_precision) is gone from
    both headers, the bindings and the library."""
    import ctypes

    from rvcx import _lib
    from rvcx.engine import Engine

    product, test = header_prototypes("rvcx.h"), header_prototypes("rvcx_test.h")
    for name in MOVED_TO_TEST_HEADER:
        assert name in test and name not in product, name
        assert name in _lib.TEST_SIG and name not in _lib.SIG, name
    assert "rvcx_conv_test_desc" not in open(os.path.join(REPO, "include", "rvcx.h")).read()
    assert "} rvcx_conv_test_desc;" in open(os.path.join(REPO, "include", "rvcx_test.h")).read()
    gone = "rvcx_set_generator_precision"
    assert gone not in product and gone not in test and gone not in _lib.SIG and gone not in _lib.TEST_SIG
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), gone)
    assert not hasattr(Engine, "set_generator_precision")


def test_recurrence_test_entries_are_exported_and_bound():
    """rvcx_gru_bidir and rvcx_dec_source (include/rvcx_test.h): declared there and not in rvcx.h, exported, bound with
    their prototypes, an Engine method each, and refused without a context."""
    from rvcx import _lib
    from rvcx.engine import Engine

    test_h = open(os.path.join(REPO, "include", "rvcx_test.h")).read()
    declared = set(re.findall(r"^\s*int\s+(rvcx_[a-z0-9_]+)\s*\(", test_h, re.M))
    lib = _lib.load()
    for name, nargs in (("rvcx_gru_bidir", 11), ("rvcx_dec_source", 8)):
        assert name in declared and name not in header_symbols() and name not in _lib.EXPORTS
        assert name in _lib.TEST_EXPORTS and name in _lib.exported_symbols()
        fn = getattr(lib, name)
        assert len(fn.argtypes) == nargs
        assert _lib.STATUS[fn(*([None] + [0] * (nargs - 1)))] == "RVCX_E_INVALID"
    assert set(_lib.TEST_EXPORTS) <= declared
    assert callable(Engine.gru_bidir) and callable(Engine.dec_source)


def test_refinegan_kernel_entries_are_exported_and_bound():
    """rvcx_rg_resample_dw, rvcx_rg_lerp_up_cat, rvcx_rg_adain (include/rvcx_test.h): the three kernels of
    csrc/refinegan.hip, declared in the test header alone, exported, bound with their prototypes, an Engine method each,
    and refused without a context."""
    from rvcx import _lib
    from rvcx.engine import Engine

    product, test = header_prototypes("rvcx.h"), header_prototypes("rvcx_test.h")
    lib = _lib.load()
    for name, nargs in (("rvcx_rg_resample_dw", 11), ("rvcx_rg_lerp_up_cat", 13), ("rvcx_rg_adain", 13)):
        assert test.get(name) == nargs and name not in product and name not in _lib.EXPORTS
        assert name in _lib.TEST_EXPORTS and name in _lib.exported_symbols()
        fn = getattr(lib, name)
        assert len(fn.argtypes) == nargs
        assert _lib.STATUS[fn(*([None] + [0] * (nargs - 1)))] == "RVCX_E_INVALID"
    assert callable(Engine.rg_resample_dw) and callable(Engine.rg_lerp_up_cat) and callable(Engine.rg_adain)


def test_engine_refuses_without_gpu():
    import torch

    from rvcx.engine import Engine

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        Engine(0)


def _ivf_bytes(nlist=4, direct_map=0):
    import numpy as np

    from oracle import ivf

    rng = np.random.default_rng(0)
    x = rng.standard_normal((300, 64)).astype(np.float32)
    return ivf.write_ivfflat(ivf.build_ivfflat(x, nlist=nlist, nprobe=2), sparse=False, direct_map=direct_map)


def test_index_parse_accepts_a_valid_file():
    """rvcx_index_parse (host only, the parser rvcx_index_load runs) on a well-formed IndexIVFFlat image."""
    from rvcx import _lib

    info = _lib.index_parse(_ivf_bytes())
    assert info == {"d": 64, "ntotal": 300, "nlist": 4, "nprobe": 2}


def test_index_parse_rejects_wrapping_list_sizes():
    """List sizes are untrusted: sizes whose sum wraps around 2^64 to ntotal, and whose byte counts
    (size * code_size) wrap to the true byte counts, must be refused (they would drive the device scan
    over ~2^63 rows)."""
    import struct

    from rvcx import _lib

    buf = bytearray(_ivf_bytes())
    at = buf.index(b"full") + 4
    (cnt,) = struct.unpack_from("<Q", buf, at)
    sizes = list(struct.unpack_from(f"<{cnt}Q", buf, at + 8))
    evil = list(sizes)
    evil[0] = (sizes[0] + (1 << 63)) % (1 << 64)
    evil[1] = (sizes[1] + (1 << 63)) % (1 << 64)
    assert sum(evil) % (1 << 64) == sum(sizes)  # the wrapped total still matches ntotal
    struct.pack_into(f"<{cnt}Q", buf, at + 8, *evil)
    with pytest.raises(_lib.RvcxError) as e:
        _lib.index_parse(bytes(buf))
    assert e.value.code == -1 and "exceeds ntotal" in str(e.value)


def test_index_parse_rejects_huge_counts():
    """A direct-map or size-vector count whose byte size wraps (count * 8 == 0 mod 2^64) is refused before
    anything is allocated from it."""
    import struct

    from rvcx import _lib

    buf = bytearray(_ivf_bytes(direct_map=1))
    # the direct map follows the quantizer: fourcc, header (33 B), centroid count u64, centroids [4][64] f32
    at = buf.index(b"IxF2") + 4 + 33 + 8 + 4 * 64 * 4
    assert buf[at] == 1 and struct.unpack_from("<Q", buf, at + 1)[0] == 300
    struct.pack_into("<Q", buf, at + 1, 1 << 61)
    with pytest.raises(_lib.RvcxError) as e:
        _lib.index_parse(bytes(buf))
    assert e.value.code == -1 and "truncated" in str(e.value)
    buf = bytearray(_ivf_bytes())
    at = buf.index(b"full") + 4
    struct.pack_into("<Q", buf, at, (1 << 61) + 4)
    with pytest.raises(_lib.RvcxError):
        _lib.index_parse(bytes(buf))


_KNOB_PROBE = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.rvcx_config_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
buf = ctypes.create_string_buffer(4096)
n = ctypes.c_int64(0)
assert lib.rvcx_config_info(None, ctypes.cast(buf, ctypes.c_void_p), 4096, ctypes.byref(n)) == 0
print(buf.value.decode())
"""


@pytest.mark.parametrize("experimental", [False, True])
def test_env_knobs_need_the_experimental_opt_in(experimental):
    """RVCX_* tuning / arithmetic switches are honoured only with RVCX_EXPERIMENTAL=1; without it
    RVCX_CONV_MATH=f32 is ignored (the default arithmetic stays) and rvcx_config_info lists it as not honoured."""
    import json
    import os
    import subprocess
    import sys

    from rvcx import _lib

    env = {k: v for k, v in os.environ.items() if not k.startswith("RVCX_")}
    env["RVCX_CONV_MATH"] = "f32"
    env["RVCX_NO_OVERLAP"] = "1"
    if experimental:
        env["RVCX_EXPERIMENTAL"] = "1"
    out = subprocess.run([sys.executable, "-c", _KNOB_PROBE, _lib.LIB_PATH], env=env, capture_output=True, text=True,
                         timeout=120, check=True).stdout
    info = json.loads(out.strip().splitlines()[-1])
    assert info["experimental"] is experimental
    assert info["conv_math_default"] == ("f32" if experimental else "h16")
    assert info["env"]["RVCX_CONV_MATH"] == {"value": "f32", "honoured": experimental}
    assert info["env"]["RVCX_NO_OVERLAP"]["honoured"] is experimental
