"""Dev tool: are the gfx950 code objects of two built trees the same machine code?  For a refactor that must not move an instruction.

Compares, kernel by kernel, the instruction text (llvm-objdump -d without addresses and encodings) and the kernel descriptor's
resources (VGPRs, AGPRs, SGPRs, LDS, scratch) of
  * the code objects inside every csrc/*.o of the two trees, and
  * with --jit, the run-time compiled kernels of the shapes build() pre-warms: every mode of lqmpc_jit_compile (solve, rollout, max-V_N,
    sweep, probe) and the controller's factor and step modes, compiled by each tree's own library into a scratch directory (needs no
    GPU).  (The controller's rollout kernel has an entry point of its own, lqmpc_jit_compile_controller_rollout, and is not compiled here.)
Prints one line per kernel: "identical", or the number of differing lines and the resources that moved.

usage: python tools/codeobj_diff.py PARENT_TREE CANDIDATE_TREE [--jit] [--jobs 8]      (both trees built: make -C lq_mpc_amd/csrc)"""
import argparse
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dpp_check import OBJDUMP, code_objects  # noqa: E402

READELF = os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf")
RES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")
JIT_MODES = ("solve", "rollout", "maxvn", "sweep", "probe", "ctl_factor", "ctl_step")
_CHILD = """
import os, sys
sys.path.insert(0, sys.argv[1])
from lq_mpc_amd import _lib
nx, nu, N, ctl, out = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
L = _lib.lib()
assert L.lqmpc_jit_cache_dir(out.encode()) == 0
_lib.jit_compile(nx, nu, N)
if ctl:
    _lib.jit_compile_controller(nx, nu, N)
"""


def kernels(obj):
    """{function name: (instruction lines, resources)} of one code object: the kernels and the device functions left out of line (no resources)."""
    text, cur = {}, None
    for ln in subprocess.run([OBJDUMP, "-d", obj], capture_output=True, text=True, check=True).stdout.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = text.setdefault(m.group(1), [])
        elif cur is not None and ln.startswith("\t"):
            txt = ln.split("//")[0].strip()
            if cur and cur[-1].startswith("s_getpc_b64") and txt.startswith("s_add_u32"):
                txt = txt.rsplit(",", 1)[0] + ", <pc-relative>"      # the distance to another function of the code object: moves with its neighbours
            cur.append(txt)
    for lines in text.values():
        # padding behind a function's last instruction (alignment of the next function; 256 s_nop behind the last function of the code
        # object): never executed, and it moves when a function is added elsewhere in the file
        while len(lines) > 1 and lines[-1] == "s_nop 0" and lines[-2].split()[0] in ("s_nop", "s_endpgm", "s_setpc_b64"):
            lines.pop()
    res, name, vals = {}, None, {}
    for ln in subprocess.run([READELF, "--notes", obj], capture_output=True, text=True, check=True).stdout.splitlines():
        m = re.match(r"\s*-?\s*(\.[a-z_]+):\s*(\S+)", ln)
        if not m:
            continue
        if m.group(1) == ".name" and not ln.startswith("        "):      # (argument names sit deeper)
            name = m.group(2).strip("'")
        elif m.group(1) in RES:
            vals[m.group(1)] = m.group(2)
        elif m.group(1) == ".wavefront_size" and name:                   # last key of a kernel's record
            res[name], name, vals = vals, None, {}
    return {k: (v, res.get(k, {})) for k, v in text.items() if v}


def compare(label, a_objs, b_objs, out):
    """code objects pairwise in order; returns (kernels, identical ones)"""
    n = same = 0
    if len(a_objs) != len(b_objs):
        out.append(f"{label}: {len(a_objs)} code objects against {len(b_objs)}")
        return 1, 0
    for a, b in zip(a_objs, b_objs):
        ka, kb = kernels(a), kernels(b)
        for name in sorted(set(ka) | set(kb)):
            n += 1
            shown = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("lqmpc::", "")
            shown = re.sub(r"\(.*", "", shown)
            if name not in ka or name not in kb:
                out.append(f"{label}: {shown}: only in the {'parent' if name in ka else 'candidate'}")
                continue
            (ta, ra), (tb, rb) = ka[name], kb[name]
            moved = [f"{k[1:]} {ra.get(k)} -> {rb.get(k)}" for k in RES if ra.get(k) != rb.get(k)]
            if ta == tb and not moved:
                same += 1
                out.append(f"{label}: {shown}: identical ({len(ta)} instructions" + "".join(f", {k[1:].split('_')[0]} {ra[k]}" for k in RES if k in ra) + ")")
            else:
                d = sum(1 for ln in difflib.unified_diff(ta, tb, lineterm="", n=0) if ln[:1] in "+-" and ln[:3] not in ("+++", "---"))
                # every resource before and after, moved or not (a kernel's own record; device functions left out of line have none)
                full = [f"{k[1:].split('_')[0]} {ra.get(k)} -> {rb.get(k)}" for k in RES if k in ra or k in rb]
                out.append(f"{label}: {shown}: DIFFERS: {d} diff lines ({len(ta)} -> {len(tb)} instructions)" + ("; " + ", ".join(moved) if moved else "")
                           + (" [" + ", ".join(full) + "]" if full else ""))
    return n, same


def jit_objects(tree, work, jobs):
    """{(shape, mode): code object} compiled by the tree's own library; the modes of a shape in the order the library compiles them"""
    sys.path.insert(0, tree)
    import importlib
    ge = importlib.import_module("__graft_entry__")
    sys.path.pop(0)
    del sys.modules["__graft_entry__"]
    shapes = [(s, s in ge.JIT_PREWARM_CONTROLLER) for s in ge.JIT_PREWARM]

    def one(arg):
        (nx, nu, N), ctl = arg
        d = os.path.join(work, f"{nx}_{nu}_{N}")
        os.makedirs(d)
        subprocess.run([sys.executable, "-c", _CHILD, tree, str(nx), str(nu), str(N), str(int(ctl)), d], check=True)
        # a cached file's name is a hash (of the program text, the headers and the compiler version), so the mode is taken from the order
        # in which lqmpc_jit_compile and lqmpc_jit_compile_controller write them (JIT_MODES restates it); checked as far as it can be:
        # the count, distinct time stamps, and the probe -- the one kernel launched with PROBE_WG = 256 threads -- where the order says it is
        files = sorted(glob.glob(os.path.join(d, "*.hsaco")), key=lambda f: os.stat(f).st_mtime_ns)
        stamps = [os.stat(f).st_mtime_ns for f in files]
        assert len(files) == (7 if ctl else 5) and len(set(stamps)) == len(stamps), (arg, files, stamps)
        wgs = [re.search(r"\.max_flat_workgroup_size:\s*(\d+)", subprocess.run([READELF, "--notes", f], capture_output=True, text=True, check=True).stdout).group(1)
               for f in files]
        assert [x == "256" for x in wgs] == [m == "probe" for m in JIT_MODES[:len(files)]], (arg, wgs)
        return {((nx, nu, N), m): f for m, f in zip(JIT_MODES, files)}
    found = {}
    with ThreadPoolExecutor(jobs) as ex:
        for r in ex.map(one, shapes):
            found.update(r)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("candidate")
    ap.add_argument("--jit", action="store_true")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    trees = [os.path.abspath(a.parent), os.path.abspath(a.candidate)]
    out, n, same, tmps = [], 0, 0, []
    for o in sorted(glob.glob(os.path.join(trees[0], "lq_mpc_amd", "csrc", "*.o"))):
        pair = []
        for t in trees:
            objs, tmp = code_objects(os.path.join(t, "lq_mpc_amd", "csrc", os.path.basename(o)))
            pair.append(objs)
            tmps.append(tmp)
        k, s = compare(os.path.basename(o), pair[0], pair[1], out)
        n, same = n + k, same + s
    if a.jit:
        work = tempfile.mkdtemp(prefix="lqmpc_codeobj_")
        tmps.append(work)
        ja, jb = (jit_objects(t, os.path.join(work, side), a.jobs) for t, side in zip(trees, ("parent", "candidate")))
        for key in sorted(ja):
            (nx, nu, N), mode = key
            k, s = compare(f"run-time compiled ({nx},{nu},{N}) {mode}", [ja[key]], [jb[key]], out)
            n, same = n + k, same + s
    print("\n".join(out))
    print(f"{n} kernels compared, {same} identical, {n - same} different")
    for t in tmps:
        if t:
            shutil.rmtree(t, ignore_errors=True)
    sys.exit(0 if n == same else 1)


if __name__ == "__main__":
    main()
