"""CPU: the resources of the page-tile compositor's two instantiations (csrc/mixed_kernels.hip, paste_tiles_kernel<CELLS_ONLY>), as the compiler
reports them for gfx950 under build.sh's own flags.  The conditions are DESIGN.md §3's: no scratch, four waves per SIMD, and the LDS each states —
the cell's taps alone (2560 bytes) where only cells are pasted, the taps and the curve's 32 segments (2560 + 3584 bytes) for regions of every kind:
the instantiation for cells must not pay for the kinds it has compiled out."""
import os
import re
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marconet_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = {"scratch": r"ScratchSize \[bytes/lane\]", "waves": r"Occupancy \[waves/SIMD\]", "lds": r"LDS Size \[bytes/block\]"}


def test_both_instantiations_keep_four_waves_no_scratch_and_their_own_lds(tmp_path):
    sh = open(os.path.join(CSRC, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', sh, flags=re.M).group(1).split()
    extra = re.search(r'mixed_kernels\) echo "([^"]*)"', sh).group(1).split()
    r = subprocess.run([HIPCC] + flags + extra + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "mixed_kernels.hip"),
                        "-o", str(tmp_path / "mixed_kernels.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    # one block of remarks per kernel: "Function Name: <mangled>", then one remark per figure
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    found = {}
    for b in blocks:
        m = re.match(r"\S*paste_tiles_kernelILb([01])E", b)
        assert m, b[:200]                                                                       # the unit holds no other kernel
        found[m.group(1) == "1"] = {k: int(re.search(pat + r": (\d+)", b).group(1)) for k, pat in FIELDS.items()}
    assert sorted(found) == [False, True], sorted(found)
    print(found)
    for cells_only, lds in ((True, 2560), (False, 6144)):
        got = found[cells_only]
        assert got["scratch"] == 0 and got["waves"] >= 4 and got["lds"] == lds, (cells_only, got)
