"""Static resource usage of the shipped kernels: `hipcc -Rpass-analysis=kernel-resource-usage` over the library's translation units with the
flags of fadtk_amd/build.py, one line per kernel (VGPRs, AGPRs, scratch bytes per lane, static LDS bytes, waves per SIMD, and the SGPRs and
VGPRs the compiler spilled: SGPRs go to VGPR lanes, VGPRs to scratch).
    python scripts/kernel_resources.py [substring ...] > profiles/rNN_kernel_resources.txt
    python scripts/kernel_resources.py nn_test > profiles/nn_test_kernel_resources.txt
`nn_test` stands for the kernels of fad_nn_test and the ones they sit beside, `kid` for those of fad_kid / fad_kid_subsets and their
Gaussian twins, `kmeans` for the kernels fad_kmeans launches (GROUPS).  No GPU needed (hipcc cross-compiles gfx950)."""
import re, subprocess, sys, pathlib
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
from fadtk_amd import build as B

GROUPS = {"nn_test": ["nearest_self_kernel", "nn_vote_kernel", "nearest_cross_kernel", "nearest_reduce_kernel", "prdc_"],
          "kid": ["kid_", "kad_pass_kernel", "kad_slots_sum_kernel"],
          "kmeans": ["kmeans::", "nearest_cross_kernel", "nearest_reduce_kernel", "kad_pack_kernel", "scatter_pairs_kernel"]}
want = [n for w in sys.argv[1:] for n in GROUPS.get(w, [w])]
src = sorted((pathlib.Path(B.__file__).parent / "csrc").glob("*.hip"))
if want and all(w in GROUPS for w in sys.argv[1:]):
    src = [s for s in src if s.name == "kad.hip"]              # every group's kernels live in kad.hip
print("# hipcc -Rpass-analysis=kernel-resource-usage (gfx950, the flags of fadtk_amd/build.py): registers, scratch, LDS and occupancy")
print("kernel | VGPRs | AGPRs | scratch B/lane | LDS B (static) | waves/SIMD | file | SGPRs spilled | VGPRs spilled")
for s in src:
    r = subprocess.run([B._hipcc(), *B.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", str(s), "-o", "/dev/null"], capture_output=True, text=True)
    cur = {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m: continue
        k, v = m.group(1), m.group(2).strip()
        if k == "Function Name":
            cur = {"name": v}
        else:
            cur[k if k.endswith("Spill") else k.split(" ")[0]] = v
        if k.startswith("LDS"):
            name = subprocess.run(["c++filt", cur["name"]], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"\(.*\)$", "", name.replace("(anonymous namespace)::", ""))
            if "anchor" in name or (want and not any(w in name for w in want)): continue
            print(f"{name} | {cur.get('VGPRs')} | {cur.get('AGPRs')} | {cur.get('ScratchSize')} | {cur.get('LDS')} | {cur.get('Occupancy')} | {s.name} | {cur.get('SGPRs Spill')} | {cur.get('VGPRs Spill')}")
