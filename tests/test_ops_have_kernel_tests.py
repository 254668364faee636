"""Every public wrapper of domain_rag_amd/ops.py that launches a kernel is called, by name, from some tests/test_gpu_*.py.

A kernel reached only through a whole-pipeline test is checked at that pipeline's tolerance (a few percent of a bf16 image), which cannot
see an indexing or rounding slip in a small kernel.  This test keeps the next wrapper from landing without a test of its own.  It reads
Python sources only (no GPU, no library)."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# wrappers that launch nothing: each with the reason it needs no kernel test
LAUNCHES_NOTHING = {
    "set_recorder": "installs the Python-side GemmRecorder; no library call",
    "set_option": "writes one entry of the library's switch table (tests/test_options.py)",
    "get_option": "reads one entry of the library's switch table (tests/test_options.py)",
    "options": "context manager over set_option / get_option",
    "experiments_built": "a query of how the library was compiled",
    "gemm_cost": "the tile policy's cost model, evaluated on the host",
    "gemm_workspace": "registers a buffer with the library; the split-K launches that use it are gemm's",
}


def _public_functions():
    tree = ast.parse(open(os.path.join(ROOT, "domain-rag_amd", "ops.py")).read())
    return [n.name for n in tree.body if isinstance(n, ast.FunctionDef) and not n.name.startswith("_")]


def test_every_launching_wrapper_is_called_by_a_gpu_test():
    names = _public_functions()
    assert len(names) > 40 and "gemm" in names and "image_preprocess" in names       # the walk itself found the file's functions
    text = "\n".join(open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))))
    missing = [n for n in names if n not in LAUNCHES_NOTHING and not re.search(r"\bops\." + re.escape(n) + r"\(", text)]
    assert not missing, f"ops wrappers that no tests/test_gpu_*.py calls: {missing}"


def test_allow_list_names_exist():
    names = set(_public_functions())
    stale = sorted(set(LAUNCHES_NOTHING) - names)
    assert not stale, f"allow-list entries that ops.py no longer defines: {stale}"
