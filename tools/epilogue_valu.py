"""static instruction counts of the epilogues of the packed sub-rectangle convolution, from the disassembly (no GPU needed):
    epilogue_valu.py <libsnake_engine.so | conv_split.o> [kernel substring, default k_conv3x3_f16s_rectp]
A kernel holds one body per tile count (a wave-uniform switch); a body's epilogue is what follows its last MFMA.  Printed per
kernel: every stretch of at least 150 instructions without an MFMA that follows an MFMA, with its vector ALU, LDS, vector memory
and scalar instruction counts (the stretches come in the order of the code: the 1-tile body's has one pass, the 8-tile body's four)."""
import os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import store_hazard_scan as shs

path = sys.argv[1]
flt = sys.argv[2] if len(sys.argv) > 2 else "k_conv3x3_f16s_rectp"
with tempfile.TemporaryDirectory() as wd:
    text = "".join(shs.disassemble(o) for o in shs.code_objects(path, wd))
cur, body = None, {}
for ln in text.splitlines():
    m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
    if m:
        cur = m.group(1)
        body[cur] = []
    elif cur and ln.startswith("\t"):
        body[cur].append(ln.split()[0])
for name, ins in body.items():
    if flt not in name or not ins:
        continue
    demangled = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    print(f"{demangled}: {len(ins)} instructions, {sum(i.startswith('v_mfma') for i in ins)} MFMAs")
    k, seen_mfma = 0, False
    while k < len(ins):
        if ins[k].startswith("v_mfma"):
            seen_mfma = True
            k += 1
            continue
        e = k
        while e < len(ins) and not ins[e].startswith("v_mfma"):
            e += 1
        run = ins[k:e]
        if seen_mfma and len(run) >= 150:
            valu = sum(i.startswith("v_") for i in run)
            cvt = sum(i.startswith(("v_cvt", "v_cndmask", "v_cmp", "v_mad_u", "v_mad_i", "v_mul_lo", "v_mul_f32")) for i in run)
            lds = sum(i.startswith("ds_") for i in run)
            vmem = sum(i.startswith(("global_", "buffer_", "flat_", "scratch_")) for i in run)
            print(f"  stretch of {len(run):5d}: vector ALU {valu:5d} (converts, selects, compares, integer multiplies {cvt:4d})  LDS {lds:4d}  "
                  f"vector memory {vmem:4d}  scalar {sum(i.startswith('s_') for i in run):4d}")
        k = e
