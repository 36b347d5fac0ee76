"""Compile csrc/okp_igemm.hip (or the file given) with the build's flags and resource remarks and print a table."""
import re, subprocess, sys, os, tempfile
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from object_keypoints_amd.build import AGPR_FILES, CFLAGS, HIPCC, RESOURCE_KEYS, RESOURCE_REMARKS, VGPR_FORM, _parse_resources  # noqa: E402
src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "object_keypoints_amd/csrc/okp_igemm.hip")
form = [] if os.path.basename(src) in AGPR_FILES else VGPR_FORM
with tempfile.TemporaryDirectory() as tmp:
    cmd = [HIPCC] + CFLAGS + form + RESOURCE_REMARKS + os.environ.get("OKP_EXTRA_CFLAGS", "").split() + ["-c", src, "-o", os.path.join(tmp, "_kres.o")]
    out = subprocess.run(cmd, capture_output=True, text=True).stderr
rows = _parse_resources(out, dict(RESOURCE_KEYS, **{"LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occ"}))
for k, v in rows.items():
    if "DF16b" in k or "okp_fire" in k or len(sys.argv) > 2:
        name = re.sub(r"_ZN12_GLOBAL__N_116okp_igemm_kernelI|EEv14OkpIgemmParams", "", k)
        print(f"{name:48s} VGPR {v.get('vgprs', -1):4d} AGPR {v.get('agprs', -1):4d} spill {v.get('vgpr_spill', -1):3d} scratch {v.get('scratch', -1):4d} LDS {v.get('lds', -1):7d} occ {v.get('occ', -1)}")
