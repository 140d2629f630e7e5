"""Static instruction census of the kernels of one HIP translation unit (slow multiplies, divisions, LDS shuffles, DPP):
    python tools/isa_stats.py ehr_vbuf.hip [kernel-name-substring ...]
--loads: instead of the census, the memory requests and the waits of the named kernels in program order -- every
`global_*` and `s_load_*` line, every `s_waitcnt` and `s_barrier`, with the basic-block labels between them:
    python tools/isa_stats.py ehr_vbuf.hip --loads vb_composite_kernelILb1ELb0ELb0ELb0
Extra hipcc flags (e.g. -DNAME=value) pass through."""
import os, re, subprocess, sys
from collections import Counter
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "easyhec_amd", "csrc")
out = "/tmp/isa_stats.s"
loads = "--loads" in sys.argv
flags = [a for a in sys.argv[2:] if a.startswith("-") and a != "--loads"]
keys = [a for a in sys.argv[2:] if not a.startswith("-")]
subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-mllvm",
                       "-amdgpu-use-amdgpu-trackers=1"] + flags + ["-S", "--cuda-device-only", sys.argv[1], "-o", out], cwd=CSRC,
                      stderr=subprocess.DEVNULL)
s = open(out).read()
for m in re.finditer(r"\n(_ZN3ehr\S+):\s*; @", s):
    n = m.group(1)
    if keys and not any(k in n for k in keys):
        continue
    i = m.start()
    j = s.index(".Lfunc_end", i)
    f = s[i:j]
    if loads:
        print(n)
        label = None
        for line in f.splitlines():
            t = line.split(";")[0].rstrip()
            if re.match(r"^\.LBB\S+:", t):
                label = t
            elif re.match(r"^\s+(global_|s_load_|s_waitcnt|s_barrier)", t):
                if label:
                    print(label)
                    label = None
                print("   ", " ".join(t.split()))
        continue
    c = Counter(re.findall(r"^\s+((?:v|s|ds|global|scratch|buffer)_[a-z0-9_]+)", f, re.M))
    print(re.sub(r"^_ZN3ehrL?\d+", "", n)[:34], "instr", sum(c.values()), "| bpermute", c["ds_bpermute_b32"], "swizzle", c["ds_swizzle_b32"],
          "dpp", len(re.findall(r"row_shr|row_ror|quad_perm|row_bcast|row_mirror|row_half", f)), "| mul_lo", c["v_mul_lo_u32"],
          "mul_hi", c["v_mul_hi_u32"] + c["v_mul_hi_i32"], "mad64", c["v_mad_u64_u32"] + c["v_mad_i64_i32"], "| int-div", c["v_rcp_iflag_f32_e32"],
          "f-div", c["v_div_scale_f32"] // 2, "| readlane", c["v_readlane_b32"], "writelane", c["v_writelane_b32"], "nop", c["s_nop"])
