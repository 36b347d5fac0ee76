"""Build recipe for libokp_hip.so (gfx950 only, in-tree so it travels with the repo snapshot).

    python -m object_keypoints_amd.build [--force]

hipcc cross-compiles without a GPU; each .hip is compiled to build/*.o in parallel and linked
into object_keypoints_amd/lib/libokp_hip.so.
"""
import concurrent.futures
import json
import os
import re
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB_DIR = os.path.join(PKG, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libokp_hip.so")
TORCH_LIB_PATH = os.path.join(LIB_DIR, "libokp_torch.so")      # torch.ops.okp.*: dispatcher shim over the same C ABI (csrc/okp_torch.cpp)
OBJ_DIR = os.path.join(REPO, "build", "okp")
ARCH = "gfx950"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CFLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-I" + os.path.join(REPO, "include"), "-I" + CSRC,
          "-Wall", "-Wno-unused-function"]
# keep MFMA accumulators in arch VGPRs: with 256-thread workgroups hipcc otherwise allocates them as
# AGPRs and copies all of them to and from VGPRs around every K-step (v_accvgpr_write/read x 128).
VGPR_FORM = ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
AGPR_FILES = set()
# per-kernel register / scratch report of the device compile (remarks only: the code is the same): build() checks that no range-guarded
# float16 instantiation (the `bool G` kernels, include/okp.h okp_conv_set_range_flag) spills
RESOURCE_REMARKS = ["-Rpass-analysis=kernel-resource-usage"]


def _sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _deps():
    return [os.path.join(REPO, "include", "okp.h"), os.path.join(CSRC, "okp_internal.h"),
            os.path.join(CSRC, "okp_igemm_kernel.h"), os.path.join(CSRC, "okp_pose_math.h"), os.path.join(CSRC, "okp_window_ring.h"),
            os.path.join(CSRC, "okp_stamps.h"), os.path.abspath(__file__)]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


RESOURCE_KEYS = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill"}


def _parse_resources(stderr, keys=RESOURCE_KEYS):
    """-Rpass-analysis=kernel-resource-usage remarks -> {kernel symbol: {"vgprs", "agprs", "scratch", "vgpr_spill", "sgpr_spill"}}
    (keys: remark name -> name in the result; scripts/kernel_resources.py asks for LDS and occupancy as well)."""
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: +([A-Za-z][A-Za-z \[\]/]*?): (\d+)(?: \[-Rpass[^\]]*\])?\s*$", line)
        if m and cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return out


def _without_remarks(stderr):
    """The compiler's console output without the resource remarks (they go to the report) and the source excerpts printed under them."""
    keep, held, in_remark = [], [], False
    for line in stderr.splitlines():
        if line.startswith("In file included from"):
            held.append(line)                  # (kept only if what follows is not a remark)
            continue
        if "remark:" in line:
            in_remark, held = True, []
            continue
        if in_remark and re.match(r"^\s*(\d+ )?\|", line):
            continue
        in_remark = False
        keep += held + [line]
        held = []
    return "\n".join(keep)


def _guarded_f16(symbol):
    """A range-guarded float16 instantiation: an fp16 kernel whose last template argument is the guard, true."""
    return "DF16_" in symbol and "Lb1EEEv" in symbol


def kernel_resources():
    """{kernel symbol: resources} of every kernel of the last build (from the compile remarks)."""
    res = {}
    for f in sorted(os.listdir(OBJ_DIR)) if os.path.isdir(OBJ_DIR) else []:
        if f.endswith(".o.res.json"):
            with open(os.path.join(OBJ_DIR, f)) as fh:
                res.update(json.load(fh))
    return res


def guarded_resources():
    """{kernel symbol: resources} of every range-guarded float16 instantiation of the last build."""
    return {k: v for k, v in kernel_resources().items() if _guarded_f16(k)}


def guarded_spills():
    """[(guarded symbol, its VGPR spills, its unguarded sibling's VGPR spills or None)] of the guarded instances that spill VGPRs."""
    res = kernel_resources()
    out = []
    for k, v in sorted(res.items()):
        if _guarded_f16(k) and v.get("vgpr_spill", 0):
            sib = res.get(k.replace("Lb1EEEv", "Lb0EEEv"))
            out.append((k, v["vgpr_spill"], sib.get("vgpr_spill", 0) if sib is not None else None))
    return out


def _compile(src):
    obj = os.path.join(OBJ_DIR, os.path.basename(src)[:-4] + ".o")
    extra = [] if os.path.basename(src) in AGPR_FILES else VGPR_FORM
    flags = CFLAGS + extra + RESOURCE_REMARKS + os.environ.get("OKP_EXTRA_CFLAGS", "").split()
    stamp = obj + ".flags"                      # an object built with other flags (experiment switches) is stale
    same_flags = os.path.exists(stamp) and open(stamp).read() == " ".join(flags)
    if not same_flags or _stale(obj, [src] + _deps()):
        cmd = [HIPCC] + flags + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
        with open(stamp, "w") as f:
            f.write(" ".join(flags))
        with open(obj + ".res.json", "w") as f:
            json.dump(_parse_resources(r.stderr), f)
        return obj, True, _without_remarks(r.stderr)
    return obj, False, ""


def build_torch_ops(verbose=False):
    """g++ (host only) build of csrc/okp_torch.cpp against this interpreter's torch: registers torch.ops.okp.* on top of the
    extern "C" symbols of libokp_hip.so (found next to it through an $ORIGIN rpath).  No HIP code, no GPU needed."""
    import torch
    from torch.utils import cpp_extension
    src = os.path.join(CSRC, "okp_torch.cpp")
    if not _stale(TORCH_LIB_PATH, [src, os.path.join(REPO, "include", "okp.h"), LIB_PATH, os.path.abspath(__file__)]):
        return TORCH_LIB_PATH
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", src, "-o", TORCH_LIB_PATH,
           "-I" + os.path.join(REPO, "include"), f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}"]
    cmd += ["-I" + p for p in cpp_extension.include_paths()]
    cmd += ["-L" + tlib, "-ltorch", "-ltorch_cpu", "-lc10", "-L" + LIB_DIR, "-lokp_hip", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + tlib]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building libokp_torch.so failed:\n{r.stdout}\n{r.stderr}")
    if verbose and r.stderr.strip():
        print(r.stderr, file=sys.stderr)
    return TORCH_LIB_PATH


def build(force=False, verbose=False):
    os.makedirs(OBJ_DIR, exist_ok=True)
    os.makedirs(LIB_DIR, exist_ok=True)
    if force:
        for f in os.listdir(OBJ_DIR):
            os.remove(os.path.join(OBJ_DIR, f))
    srcs = _sources()
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(4, len(srcs))) as ex:
        results = list(ex.map(_compile, srcs))
    objs = [o for o, _, _ in results]
    rebuilt = any(r for _, r, _ in results)
    for f in os.listdir(OBJ_DIR):                 # objects (and flag stamps) of sources that no longer exist
        if f.endswith((".o", ".o.flags", ".o.res.json")) and os.path.join(OBJ_DIR, f.split(".o")[0] + ".o") not in objs:
            os.remove(os.path.join(OBJ_DIR, f))
    if verbose:
        for _, _, err in results:
            if err.strip():
                print(err, file=sys.stderr)
    if rebuilt or _stale(LIB_PATH, objs):
        cmd = [HIPCC, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", LIB_PATH] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    guarded = guarded_resources()
    # (VGPR spills go to scratch memory; SGPR spills land in VGPR lanes, as in the unguarded instances.)  A guarded instance whose
    # unguarded sibling does not spill is a regression of this build; one whose sibling already spills (the 32x32 A/B tiles, the stem) is listed
    spills = guarded_spills()
    new = [f"{k} ({n})" for k, n, sib in spills if not sib]
    if new:
        print("warning: range-guarded float16 instantiations that spill VGPRs where the unguarded one does not: " + ", ".join(new), file=sys.stderr)
    if verbose and guarded:
        old = ", ".join(f"{k} ({n}; unguarded {sib})" for k, n, sib in spills if sib)
        print(f"range-guarded float16 instantiations: {len(guarded)}, {len(new)} spilling where the unguarded sibling does not"
              + (f"; spilling as their unguarded siblings do: {old}" if old else ""), file=sys.stderr)
    try:
        build_torch_ops(verbose)
    except Exception as e:        # the dispatcher shim is optional: the ctypes binding serves every launch without it
        if os.path.exists(TORCH_LIB_PATH):
            os.remove(TORCH_LIB_PATH)          # never leave a stale shim built against another torch / ABI
        print(f"warning: libokp_torch.so (torch.ops.okp.*) not built, the ctypes binding will be used: {e}", file=sys.stderr)
    return LIB_PATH


if __name__ == "__main__":
    path = build(force="--force" in sys.argv, verbose=True)
    print(path)
