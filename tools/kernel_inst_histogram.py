#!/usr/bin/env python3
"""Static instruction counts of the kernels in a device assembly file (hipcc -S --cuda-device-only, or the gemm-*-gfx950.s that
the build keeps): for every kernel whose mangled name matches PATTERN, the instructions between its label and s_endpgm.

    python tools/kernel_inst_histogram.py licv-vqa_amd/csrc/build/gemm-hip-amdgcn-amd-amdhsa-gfx950.s 'flow64_k' [--top 12]

Prints one markdown row per kernel: vector-ALU instructions other than MFMAs and accumulator-file moves (v_* but v_mfma* and
v_accvgpr_*), MFMAs, accumulator-file moves, s_nop, branches, the bf16 conversions,
the SDWA ors that re-pair halves, packed-f32 instructions, and the resource record's VGPR / scratch figures."""
import argparse
import collections
import re
import subprocess


def demangle(name):
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True, check=True).stdout.strip().split("(")[0].replace("void ", "")
    except Exception:
        return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("pattern")
    ap.add_argument("--top", type=int, default=0, help="also print the N most frequent mnemonics of each kernel")
    args = ap.parse_args()
    text = open(args.asm).read()
    print("| kernel | VALU | MFMA | accvgpr moves | s_nop | branches | v_cvt_pk_bf16_f32 | v_or_b32_sdwa | v_pk_*_f32 | arch VGPRs | scratch B |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*s_endpgm(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        name, body, meta = m.groups()
        if not re.search(args.pattern, name):
            continue
        hist = collections.Counter()
        for line in body.splitlines():
            t = line.split(";")[0].strip()
            if not t or t.startswith(".") or t.endswith(":"):
                continue
            hist[t.split()[0]] += 1
        valu = sum(n for k, n in hist.items() if k.startswith("v_") and not k.startswith(("v_mfma", "v_accvgpr")))
        accm = sum(n for k, n in hist.items() if k.startswith("v_accvgpr"))
        mfma = sum(n for k, n in hist.items() if k.startswith("v_mfma"))
        br = sum(n for k, n in hist.items() if k.startswith("s_cbranch") or k == "s_branch")
        pk = sum(n for k, n in hist.items() if re.match(r"v_pk_\w+_f32", k))
        vg = re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta)
        acc = re.search(r"\.amdhsa_accum_offset (\d+)", meta)
        sc = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta)
        print(f"| `{demangle(name)}` | {valu} | {mfma} | {accm} | {hist['s_nop']} | {br} | {hist['v_cvt_pk_bf16_f32']} | {hist['v_or_b32_sdwa']} | {pk} | "
              f"{acc.group(1) if acc else (vg.group(1) if vg else '?')} | {sc.group(1) if sc else '?'} |")
        if args.top:
            print("  " + ", ".join(f"{k} {n}" for k, n in hist.most_common(args.top)))


if __name__ == "__main__":
    main()
