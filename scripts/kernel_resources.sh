#!/bin/bash
# usage: scripts/kernel_resources.sh bilevel-gait-gen_amd/libsrbm_rti.so  -> per kernel of EVERY gfx950 code object of the library (one per .hip
# source: srbm_capi.hip, which includes the kernels of csrc/*.hiph -- the IPM's are srbm_k3_lds / _rows / _normal / _ipm.hiph, the gait step's srbm_gait_candidates / _sens / _grad / _lp.hiph, the linearised model srbm_lin.hiph): VGPRs, AGPRs, SGPRs, spills, scratch bytes per lane, static LDS and a short
# hash of its disassembly; per out-of-line device function the hash alone.  Lines sorted by name.  The hash drops the `//` comments (addresses,
# encodings) and masks the literal of every s_add_u32 / s_addc_u32 within three instructions after an s_getpc_b64: those are PC-relative
# offsets, which change whenever any function moves in the code object; the padding after a function (s_nop, zero bytes) is dropped too.  Two builds whose outputs
# agree have the same instructions: `diff` the listing of the parent's build with the branch's, for each library (scripts/README.md).
LIB=$1
T=$(mktemp -d)
/opt/rocm/lib/llvm/bin/llvm-objcopy -O binary --only-section=.hip_fatbin $LIB $T/fat.bin
python3 - $T <<'PY'
import hashlib, re, subprocess, sys
T = sys.argv[1]
d = open(T + '/fat.bin', 'rb').read()
offs = [m.start() for m in re.finditer(b'__CLANG_OFFLOAD_BUNDLE__', d)]

def isa_hashes(co):
    asm = subprocess.check_output(['/opt/rocm/lib/llvm/bin/llvm-objdump', '-d', '--no-show-raw-insn', '--no-leading-addr', co]).decode()
    funcs, name, since_getpc = {}, None, 99
    for line in asm.splitlines():
        m = re.match(r'^<(.+)>:$', line)
        if m:
            name, since_getpc = m.group(1), 99
            funcs[name] = []
            continue
        ins = line.split('//')[0].strip()
        if name is None or not ins:
            continue
        since_getpc += 1
        if ins.startswith('s_getpc_b64'):
            since_getpc = 0
        elif since_getpc <= 3 and re.match(r's_addc?_u32 ', ins):
            ins = re.sub(r',\s*(0x[0-9a-fA-F]+|-?\d+)$', ', LIT', ins)
        funcs[name].append(ins)
    for v in funcs.values():                      # the padding after a function: s_nop, or zero bytes (objdump prints them as `...`)
        while v and (v[-1].startswith('s_nop') or v[-1] == '...'):
            v.pop()
    return {n: hashlib.sha1('\n'.join(v).encode()).hexdigest()[:12] for n, v in funcs.items()}

for i, o in enumerate(offs):
    end = offs[i + 1] if i + 1 < len(offs) else len(d)
    open('%s/fat%d.bin' % (T, i), 'wb').write(d[o:end])
    co = '%s/k%d.co' % (T, i)
    subprocess.call(['/opt/rocm/lib/llvm/bin/clang-offload-bundler', '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950',
                     '--input=%s/fat%d.bin' % (T, i), '--output=' + co])
    txt = subprocess.check_output(['/opt/rocm/lib/llvm/bin/llvm-readelf', '--notes', co]).decode()
    hashes = isa_hashes(co)
    print('# code object %d of %d' % (i + 1, len(offs)))
    lines = {}
    for blk in txt.split('- .agpr_count:')[1:]:
        g = lambda k: (re.search(r'\.' + k + r':\s+(\S+)', blk) or [None, '?'])[1]
        lines[g('name')] = '%-48s vgpr %s agpr %s sgpr %s vspill %s sspill %s scratch %s lds %s isa %s' % (
            g('name')[:48], g('vgpr_count'), blk.split()[0], g('sgpr_count'), g('vgpr_spill_count'), g('sgpr_spill_count'),
            g('private_segment_fixed_size'), g('group_segment_fixed_size'), hashes.get(g('name'), '?'))
    for n, h in hashes.items():
        lines.setdefault(n, '%-48s isa %s' % (n[:48], h))
    for n in sorted(lines):
        print(lines[n])
PY
rm -rf $T
