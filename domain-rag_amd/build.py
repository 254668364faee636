"""Build libdomainrag_hip.so (gfx950 only) from csrc/*.hip with hipcc.

In-tree build: objects go to ``domain-rag_amd/build/`` and the shared library to
``domain-rag_amd/lib/libdomainrag_hip.so`` so that the built library travels with the source tree
(it is git-ignored, not gpurun-ignored).  hipcc cross-compiles without a GPU.
"""
from __future__ import annotations

import hashlib
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
BUILD = os.path.join(HERE, "build")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libdomainrag_hip.so")
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wno-unused-result",
         "-ffp-contract=on"]
# DRAG_EXPERIMENTS=1: also compile the kernels behind the experiment switches (attn_persist, attn_sched 3, topk_qt: measured
# non-improvements, kept for their A/B records — csrc/drag_common.h); the flag is part of every object's digest, so switching rebuilds
if os.environ.get("DRAG_EXPERIMENTS", "") not in ("", "0"):
    FLAGS.append("-DDRAG_EXPERIMENTS")


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: libdomainrag_hip.so cannot be built")


def _isa_check():
    spec = importlib.util.spec_from_file_location("_drag_isa_check", os.path.join(HERE, "isa_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ISA = _isa_check()


class IsaCheckError(RuntimeError):
    """a shipped object breaks one of the rules of isa_check.py (asm LDS reads / asm MFMA operands): the build stops"""


def _sources() -> list[str]:
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _included(path: str, seen: set[str] | None = None) -> list[str]:
    """the headers `path` reaches through #include "..." lines, each resolved relative to the file that names it; one that does not exist
    (attn_q64_tile_exp.h outside an experiments build, under its #if) is skipped"""
    seen = set() if seen is None else seen
    with open(path, errors="replace") as f:
        names = re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', f.read(), re.M)
    for name in names:
        h = os.path.normpath(os.path.join(os.path.dirname(path), name))
        if h not in seen and os.path.exists(h):
            seen.add(h)
            _included(h, seen)
    return sorted(seen)


def _digest(path: str, extra: list[str], compiler: str = "") -> str:
    h = hashlib.sha256()
    for p in [path] + extra:
        with open(p, "rb") as f:
            h.update(f.read())
    h.update(" ".join(FLAGS).encode())
    h.update(compiler.encode())      # another hipcc allocates registers differently around the asm statements: recompile AND re-check
    return h.hexdigest()


def _compiler_version(isa, hipcc: str) -> str:
    """`hipcc --version` is part of every object's digest; every process that loads the library calls build_library, so the string is cached
    next to the stamps, keyed on the compiler's path, size and mtime (no subprocess per load)"""
    st = os.stat(os.path.realpath(hipcc))
    key = f"{os.path.realpath(hipcc)}|{st.st_size}|{st.st_mtime_ns}"
    cache = os.path.join(BUILD, "hipcc_version.json")
    try:
        with open(cache) as f:
            d = json.load(f)
        if d.get("key") == key and d.get("version"):
            return d["version"]
    except (OSError, ValueError):
        pass
    v = isa.hipcc_version(hipcc)
    try:
        with open(cache + ".tmp", "w") as f:
            json.dump({"key": key, "version": v}, f)
        os.replace(cache + ".tmp", cache)
    except OSError:
        pass
    return v


def build_library(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(BUILD, exist_ok=True)
    os.makedirs(LIBDIR, exist_ok=True)
    hipcc = _hipcc()
    exp_header = os.path.join(CSRC, "attn_q64_tile_exp.h")
    if "-DDRAG_EXPERIMENTS" in FLAGS:
        # the generated attention stream's schedule variants (3 MB of asm text): written here, from the generator, for experiment builds only
        gen = os.path.join(HERE, "..", "scripts", "gen", "attn_q64_tile.py")
        r = subprocess.run([sys.executable, gen, "--experiments"], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{gen} --experiments failed:\n{r.stderr}")
        if not os.path.exists(exp_header) or open(exp_header).read() != r.stdout:
            with open(exp_header, "w") as f:
                f.write(r.stdout)
    isa = ISA
    compiler = _compiler_version(isa, hipcc)
    # the checker is part of what an object was built under: editing its rules re-checks (= recompiles) the checked sources
    checker = [os.path.join(HERE, "isa_check.py")]
    jobs = []
    objs = []
    for src in _sources():
        obj = os.path.join(BUILD, os.path.basename(src)[:-4] + ".o")
        stamp = obj + ".sha"
        deps = _included(src)
        dig = _digest(src, deps + (checker if os.path.basename(src) in isa.CHECKED else []), compiler)
        objs.append(obj)
        if not force and os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == dig:
            continue
        jobs.append((src, obj, stamp, dig, sum(os.path.getsize(p) for p in [src] + deps)))
    # the largest sources first (by the bytes the compiler reads: a kernel's body may live in a header), so that the longest compiles
    # start at once instead of behind the queue
    jobs.sort(key=lambda job: job[4], reverse=True)

    def compile_one(job):
        src, obj, stamp, dig = job[:4]
        base = os.path.basename(src)
        wanted = isa.CHECKED.get(base)
        if os.path.exists(stamp):
            os.remove(stamp)
        if wanted is None:
            r = subprocess.run([hipcc] + FLAGS + ["-c", src, "-o", obj], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
        else:
            # a source with inline-asm LDS reads / MFMAs: keep the device assembly THIS object is assembled from (-save-temps) and walk
            # it with the rules of isa_check.py; an object that breaks them is not shipped (VERDICT / ADVICE round 4)
            with tempfile.TemporaryDirectory(dir=BUILD) as tmp:
                tobj = os.path.join(tmp, base[:-4] + ".o")
                r = subprocess.run([hipcc] + FLAGS + ["-save-temps=obj", "-c", src, "-o", tobj], capture_output=True, text=True, cwd=tmp)
                if r.returncode != 0:
                    raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
                asm_files = [f for f in os.listdir(tmp) if f.endswith(f"{ARCH}.s")]
                if len(asm_files) != 1:
                    raise RuntimeError(f"{src}: expected one device assembly file from -save-temps, found {asm_files}")
                lines: list[str] = []
                status, seen = isa.check_asm_text(open(os.path.join(tmp, asm_files[0])).read(), wanted, out=lines.append)
                report = {"source": base, "kernels": wanted, "kernels_seen": seen, "status": status, "hipcc": compiler, "flags": FLAGS,
                          "report": lines}
                with open(os.path.join(BUILD, base[:-4] + ".isa_check.json"), "w") as f:
                    json.dump(report, f, indent=1)
                if status != 0 or seen == 0:
                    why = "no kernel matching " + repr(wanted) if seen == 0 else "the compiled code breaks a rule of isa_check.py"
                    msg = f"{src}: {why} (compiler: {compiler})\n" + "\n".join(lines)
                    if os.environ.get("DRAG_ISA_CHECK", "") == "warn" and seen != 0:
                        # explicit override (the checker documents false positives on branchy code; a compiler update must not leave an
                        # installation without a library): the object IS built, the report says so, the caller was told
                        print(f"[domain-rag_amd] WARNING, DRAG_ISA_CHECK=warn: {msg}\n[domain-rag_amd] building the object anyway", file=sys.stderr)
                        report["overridden"] = True
                        with open(os.path.join(BUILD, base[:-4] + ".isa_check.json"), "w") as f:
                            json.dump(report, f, indent=1)
                    else:
                        if os.path.exists(obj):
                            os.remove(obj)
                        raise IsaCheckError(msg + "\nobject NOT built; the previously linked library is removed (it was built from other sources or "
                                            "by another compiler).  DRAG_ISA_CHECK=warn builds it anyway after you have read the report above.")
                shutil.move(tobj, obj)
        with open(stamp, "w") as f:
            f.write(dig)
        return src

    if jobs:
        if verbose:
            print(f"[domain-rag_amd] compiling {len(jobs)} HIP source(s) for {ARCH} ...", file=sys.stderr)
        try:
            workers = int(os.environ.get("MAX_JOBS") or 8)
            with ThreadPoolExecutor(max_workers=max(1, min(workers, 16, len(jobs)))) as ex:
                list(ex.map(compile_one, jobs))
        except Exception:
            # a library linked from an earlier state of the sources must not outlive a failed build of the current one
            if os.path.exists(LIB):
                os.remove(LIB)
            raise
    missing = [o for o in objs if not os.path.exists(o)]
    if missing:
        raise RuntimeError(f"objects missing after the compile step: {missing}")
    if jobs or not os.path.exists(LIB):
        cmd = [hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr}")
        # a shared object with an unresolved symbol links fine and only fails at dlopen: check now — in a CHILD
        # process, so that this process does not load the system HIP runtime before torch loads its own copy
        # (two HIP runtimes in one process = "no ROCm-capable device" on the first launch)
        r = subprocess.run([sys.executable, "-c", f"import ctypes; ctypes.CDLL({LIB!r})"], capture_output=True, text=True)
        if r.returncode != 0:
            os.remove(LIB)
            raise RuntimeError(f"libdomainrag_hip.so does not load: {r.stderr.strip().splitlines()[-1] if r.stderr else r.returncode}")
        if verbose:
            print(f"[domain-rag_amd] built {LIB}", file=sys.stderr)
    return LIB


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
