#!/usr/bin/env python3
"""Register and spill report of the wide kernels, from the compiler alone (no GPU): the -Rpass-analysis=kernel-resource-usage remark block
of every hot kernel plus, from the device assembly, the per-function counts of v_readlane_b32 / v_writelane_b32 (scalar-register spill
traffic) and scratch accesses, in all and inside loops.  Run by `make -C multi-modal-image-fusion_amd/csrc resource-usage`:
    resource_usage.py <remarks.txt> <device.s> [<remarks.txt> <device.s> ...] > profiles/wide_kernels_resource_usage.txt"""
import re, subprocess, sys

HOT = ("conv_dma_kernel", "wgrad_dma_kernel", "bwd_pair_dma_kernel", "conv_x3_kernel", "wgrad_x3_kernel")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except Exception:
        return {n: n for n in names}


def main(argv):
    print("# Wide kernels: compiler resource usage and spill traffic (hipcc -O3, gfx950, device only).  loop = inside a loop's blocks.")
    for rem_path, asm_path in zip(argv[0::2], argv[1::2]):
        rem, asm = open(rem_path).read(), open(asm_path).read()
        funcs = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)\.Lfunc_end\d+:", asm, re.S | re.M)}
        blocks = re.split(r"remark: Function Name: ", rem)[1:]
        names = [b.split()[0] for b in blocks]
        nice = demangle(names)
        for name, blk in zip(names, blocks):
            if not any(h in name for h in HOT):
                continue
            print(f"\n## {nice[name].split('(')[0]}")
            for line in blk.split("\n")[1:]:
                m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
                if m:
                    print("   ", m.group(1).strip())
            body = funcs.get(name, "")
            tot = {"v_readlane_b32": 0, "v_writelane_b32": 0, "scratch_": 0}
            inl = dict(tot)
            in_loop = False
            for l in body.split("\n"):
                if l.startswith(".LBB"):
                    in_loop = "in Loop" in l or "Loop Header" in l
                elif l.startswith("; %bb."):
                    in_loop = "in Loop" in l or "Loop Header" in l
                for k in tot:
                    if re.match(r"\s+" + k, l):
                        tot[k] += 1
                        inl[k] += in_loop
            print(f"    assembly: v_readlane_b32 {tot['v_readlane_b32']} (loop {inl['v_readlane_b32']}), v_writelane_b32 {tot['v_writelane_b32']} "
                  f"(loop {inl['v_writelane_b32']}), scratch accesses {tot['scratch_']} (loop {inl['scratch_']})")


if __name__ == "__main__":
    main(sys.argv[1:])
