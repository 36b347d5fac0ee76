"""Dump the gfx950 device assembly of csrc/*.hip (or the files given) with the build's flags and print one sha256 per file.

    python scripts/device_asm.py [--out DIR] [file.hip ...]

Two trees whose hashes agree file by file compile to the same instructions: the way to show that a source clean-up changed no
kernel.  The `__hip_cuid_<hash>` symbol hashes the source text, so it is replaced by a fixed token before hashing.  The .s files
go to DIR (default build/device_asm, which git ignores).  OKP_EXTRA_CFLAGS is honoured as in the build (stamp builds).
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from object_keypoints_amd.build import AGPR_FILES, CFLAGS, HIPCC, VGPR_FORM, _sources  # noqa: E402


def device_asm(src, out_dir):
    extra = [] if os.path.basename(src) in AGPR_FILES else VGPR_FORM
    flags = CFLAGS + extra + os.environ.get("OKP_EXTRA_CFLAGS", "").split()
    r = subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", r.stdout)
    with open(os.path.join(out_dir, os.path.basename(src)[:-4] + ".s"), "w") as f:
        f.write(text)
    return hashlib.sha256(text.encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(REPO, "build", "device_asm"))
    ap.add_argument("files", nargs="*")
    args = ap.parse_args()
    srcs = [os.path.abspath(f) for f in args.files] or _sources()
    os.makedirs(args.out, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(4, len(srcs))) as ex:
        for src, digest in zip(srcs, ex.map(lambda s: device_asm(s, args.out), srcs)):
            print(f"{digest}  {os.path.basename(src)}", flush=True)


if __name__ == "__main__":
    main()
