"""Build-time check that the order block's pair kernel keeps its register block of pairs in registers and that the easiness
kernel needs no scratch either (gfx950 ISA of csrc/order.hip).  A block that has slipped into scratch memory still gives the
right numbers, only slowly -- no numerical test can see it."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-value"]
KERNELS = ["17order_pair_kernelILi", "21order_easiness_kernel"]


def _kernels(src):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", *FLAGS, "--cuda-device-only", "-S", os.path.join(ROOT, "gpirt_amd", "csrc", src), "-o", out])
        txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S):
        body = m.group(2)
        priv = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        vg = re.search(r"\.amdhsa_next_free_vgpr (\d+)", body)
        res[m.group(1)] = (int(priv.group(1)) if priv else 0, int(vg.group(1)) if vg else None)
    return res


def test_the_pairs_stay_in_registers():
    ks = _kernels("order.hip")
    for frag in KERNELS:
        hits = [(k, v) for k, v in ks.items() if frag in k]
        assert len(hits) == 1, (frag, sorted(ks))
        for k, (scratch, vgpr) in hits:
            print(f"{k}: {scratch} bytes of scratch per lane, {vgpr} registers")
            assert scratch == 0, f"{k}: {scratch} bytes of scratch per lane ({vgpr} registers)"
