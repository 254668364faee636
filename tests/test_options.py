"""CPU-side checks of the library's tuning switches: one table (csrc/drag_common.h) behind drag_set_option / drag_get_option /
drag_option_name, initial values from $DRAG_<NAME>, and ops.options as the way to switch and restore.  Host-only: nothing launches."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPERIMENT_ONLY = {"attn_persist": 1, "topk_qt": 2, "attn_sched": 3}        # switch -> a value only a DRAG_EXPERIMENTS library accepts
DEFAULTS = {"attn_sched": 2, "attn_tune": 2}                                # every other switch starts at 0


def _names(lib):
    names = []
    while (n := lib.drag_option_name(len(names))) is not None:
        names.append(n.decode())
        assert len(names) < 1000, "drag_option_name never returns NULL"
    return names


def _get(lib, name):
    v = ctypes.c_int32(-12345)
    assert lib.drag_get_option(name.encode(), ctypes.byref(v)) == 0, lib.drag_last_error()
    return v.value


def test_every_option_is_enumerated_readable_settable_and_documented(built_lib):
    names = _names(built_lib)
    assert len(names) >= 29 and len(set(names)) == len(names)
    assert built_lib.drag_option_name(-1) is None and built_lib.drag_option_name(len(names)) is None
    header = open(os.path.join(ROOT, "include", "domainrag_hip.h")).read()
    for n in names:
        assert built_lib.drag_set_option(n.encode(), _get(built_lib, n)) == 0, n
        assert len(re.findall(r'^ \*   "%s" ' % re.escape(n), header, flags=re.M)) == 1, f'"{n}" needs exactly one line in drag_set_option\'s comment'
    for n in ("gemm_t128", "gemm_no_96", "gemm_no_192", "gemm_nonpersistent", "gemm_narrow", "conv_no_small_cout", "conv_no_lin",
              "conv_tile", "attn_gen", "gemm_epilogue"):
        assert n in names
    v = ctypes.c_int32()
    assert built_lib.drag_get_option(b"no_such_switch", ctypes.byref(v)) != 0
    msg = built_lib.drag_last_error().decode()
    assert "unknown option" in msg and all(n in msg for n in names) and msg.endswith(")")      # the whole list fits the message
    assert built_lib.drag_set_option(b"no_such_switch", 1) != 0 and b"unknown option" in built_lib.drag_last_error()


# a child that only loads the library and reads the switches: no torch, no device
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.drag_option_name.restype = ctypes.c_char_p
out, i = {}, 0
while (n := lib.drag_option_name(i)) is not None:
    v = ctypes.c_int32()
    assert lib.drag_get_option(n, ctypes.byref(v)) == 0
    out[n.decode()] = v.value
    i += 1
print(json.dumps(out))
"""


def _child_options(lib, env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRAG_")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", _CHILD, lib._name], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.splitlines()[-1])


def test_initial_values_come_from_the_environment_by_the_naming_rule(built_lib):
    """$DRAG_<NAME IN UPPER CASE> for every switch, nothing else; unset = the table's default, set but empty = 1"""
    names = _names(built_lib)
    product = [n for n in names if n not in EXPERIMENT_ONLY or n == "attn_sched"]
    want = {n: 4 + i for i, n in enumerate(product)}          # distinct, and no switch's experiment-only value
    got = _child_options(built_lib, {"DRAG_" + n.upper(): str(v) for n, v in want.items()})
    assert {n: got[n] for n in product} == want
    got = _child_options(built_lib, {})
    assert got == {n: DEFAULTS.get(n, 0) for n in names}
    got = _child_options(built_lib, {"DRAG_GEMM_T128": "", "DRAG_CONV_TILE": "0", "DRAG_GEMM_NARROW": "0"})
    assert got["gemm_t128"] == 1 and got["conv_tile"] == 0 and got["gemm_narrow"] == 0
    if not built_lib.drag_experiments_built():                # a product library ignores the experiments' variables
        got = _child_options(built_lib, {"DRAG_ATTN_PERSIST": "1", "DRAG_TOPK_QT": "2", "DRAG_ATTN_SCHED": "3"})
        assert got["attn_persist"] == 0 and got["topk_qt"] == 0 and got["attn_sched"] == 2


@pytest.mark.parametrize("option, shape, off, on", [
    ("gemm_t128", (8192, 0, 4096, 4096), 2, 0),
    ("gemm_t128", (1024, 0, 12288, 3072), 2, 0),
    ("gemm_no_96", (1024, 0, 4304, 1152), 32, 0),
    ("gemm_no_192", (512, 0, 9216, 3072), 143, 32),
    ("gemm_no_192", (512, 0, 12288, 3072), 143, 0),
])
def test_tile_policy_switches_take_effect_inside_one_process(built_lib, option, shape, off, on):
    """the switches that used to freeze at the first launch: set and cleared in ONE process, the policy query sees both (the expected codes
    were measured in fresh processes on the commit before the switches joined the table)"""
    from domain_rag_amd import ops
    c = built_lib.drag_gemm_bf16_choice
    assert c(*shape) == off
    with ops.options(**{option: 1}):
        assert c(*shape) == on
    assert c(*shape) == off
    assert all(ops.get_option(n) == 0 for n in ("gemm_t128", "gemm_no_96", "gemm_no_192"))     # test_abi's policy table holds as before


def test_options_context_restores_on_exit_and_on_exception(built_lib):
    from domain_rag_amd import ops
    names = _names(built_lib)
    ops.set_option("gemm_group_m", 4)
    try:
        before = {n: ops.get_option(n) for n in names}
        with ops.options(gemm_group_m=8, attn_sched=0, conv_tile=3):
            assert (ops.get_option("gemm_group_m"), ops.get_option("attn_sched"), ops.get_option("conv_tile")) == (8, 0, 3)
            with ops.options(attn_sched=1):
                assert ops.get_option("attn_sched") == 1
            assert ops.get_option("attn_sched") == 0
        assert {n: ops.get_option(n) for n in names} == before        # gemm_group_m back at 4: the value before, not the default
        with pytest.raises(ZeroDivisionError):
            with ops.options(gemm_kernel=1, gemm_pair=2):
                1 // 0
        assert {n: ops.get_option(n) for n in names} == before
        with pytest.raises(RuntimeError, match="unknown option"):                  # refused half way: what was already set goes back
            with ops.options(gemm_kernel=1, no_such_switch=1):
                pass
        assert {n: ops.get_option(n) for n in names} == before
        with ops.options(attn_persist=0, topk_qt=0):                               # 0 for an experiment-only switch: always accepted
            pass
    finally:
        ops.set_option("gemm_group_m", 0)


def test_product_library_refuses_the_experiments(built_lib):
    from domain_rag_amd import ops
    if ops.experiments_built():          # an experiment build accepts them
        return
    for name, v in EXPERIMENT_ONLY.items():
        before = ops.get_option(name)
        with pytest.raises(RuntimeError, match="experiments"):
            ops.set_option(name, v)
        with pytest.raises(RuntimeError, match="experiments"):
            with ops.options(**{name: v}):
                pass
        assert ops.get_option(name) == before
        assert "DRAG_EXPERIMENTS=1" in built_lib.drag_last_error().decode()


def test_only_the_option_table_reads_the_environment():
    csrc = os.path.join(ROOT, "domain-rag_amd", "csrc")
    users = sorted(f for f in os.listdir(csrc) if "getenv" in open(os.path.join(csrc, f), errors="replace").read())
    assert users == ["capi.hip"]
    assert open(os.path.join(csrc, "capi.hip")).read().count("getenv(") == 1
