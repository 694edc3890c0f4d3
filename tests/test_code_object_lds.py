"""The constant LDS base of the out-of-line device functions (SRBM_LDS_BASE, bilevel-gait-gen_amd/csrc/srbm_types.h) against the built code objects
(no GPU): in each library that is built -- libsrbm_rti.so, libsrbm_rti_large.so, the diagnostic libsrbm_rti_prof.so --

  * every kernel that reaches a device function which is not a kernel and has LDS instructions has exactly SRBM_LDS_BASE bytes of static LDS
    (group_segment_fixed_size): such a function addresses the dynamic LDS from the constant, so a kernel that gains static LDS -- its dynamic LDS
    then begins behind it -- fails here instead of running with wrong addresses;
  * the compiler's table of dynamic-LDS bases (llvm.amdgcn.dynlds.offset.table), which it emits as soon as one function that is not a kernel names
    the extern symbol srbm_lds, is not in the code object -- in the standard and the diagnostic build.  The LARGE build keeps the symbol in its
    out-of-line functions (srbm_types.h says why): there the table must be present, and the kernels' static LDS is held to the constant all the same.

The call graph is read from the disassembly: a call (or an address taken) is s_getpc_b64 followed by s_add_u32 with a literal, the target is the
address of that s_add_u32 plus the literal; targets that are function symbols are edges."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'bilevel-gait-gen_amd')
LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin')
LIBS = {'libsrbm_rti.so': False, 'libsrbm_rti_large.so': False, 'libsrbm_rti_prof.so': True}      # name -> built with -DSRBM_PROFILE
KEEPS_TABLE = {'libsrbm_rti_large.so'}            # builds whose out-of-line functions name the extern symbol (SRBM_LDS_OUT_OF_LINE is empty there)
TABLE = 'llvm.amdgcn.dynlds.offset.table'


def lds_base(profile):
    """SRBM_LDS_BASE of srbm_types.h for a build with / without -DSRBM_PROFILE"""
    text = open(os.path.join(PKG, 'csrc', 'srbm_types.h')).read()
    m = re.search(r'#ifdef SRBM_PROFILE\n#define SRBM_LDS_BASE (\d+)u\n#else\n#define SRBM_LDS_BASE (\d+)u\n#endif', text)
    assert m, 'the definition of SRBM_LDS_BASE'
    return int(m.group(1 if profile else 2))


def code_objects(lib, tmp):
    fat = os.path.join(tmp, 'fat.bin')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', lib, fat])
    data = open(fat, 'rb').read()
    offs = [m.start() for m in re.finditer(b'__CLANG_OFFLOAD_BUNDLE__', data)]
    for i, o in enumerate(offs):
        part, co = os.path.join(tmp, 'fat%d.bin' % i), os.path.join(tmp, 'k%d.co' % i)
        open(part, 'wb').write(data[o:offs[i + 1] if i + 1 < len(offs) else len(data)])
        subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950',
                               '--input=' + part, '--output=' + co])
        yield co


def analyse(co):
    """kernels {name: static LDS bytes}, functions {name: (has LDS instructions, set of callee names)}, all symbol names"""
    run = lambda *a: subprocess.check_output([os.path.join(LLVM, a[0])] + list(a[1:])).decode()
    notes = run('llvm-readelf', '--notes', co)
    kernels = {}
    for blk in notes.split('- .agpr_count:')[1:]:
        kernels[re.search(r'\.name:\s+(\S+)', blk).group(1)] = int(re.search(r'\.group_segment_fixed_size:\s+(\d+)', blk).group(1))
    symbols, at = set(), {}
    for line in run('llvm-readelf', '-sW', co).splitlines():
        f = line.split()
        if len(f) >= 8 and f[0].endswith(':') and f[0][:-1].isdigit():
            symbols.add(f[7])
            if f[3] == 'FUNC':
                at[int(f[1], 16)] = f[7]
    funcs, name, getpc = {}, None, 99
    for line in run('llvm-objdump', '-d', '--no-show-raw-insn', co).splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            name, getpc = m.group(1), 99
            funcs[name] = [False, set()]
            continue
        ins, _, comment = line.partition('//')
        ins = ins.strip()
        if name is None or not ins:
            continue
        getpc = 0 if ins.startswith('s_getpc_b64') else getpc + 1
        if ins.startswith('ds_'):
            funcs[name][0] = True
        m = re.match(r's_add_u32 \S+,\s*\S+,\s*(0x[0-9a-f]+|-?\d+)$', ins)
        if m and getpc == 1:
            lit = int(m.group(1), 0)
            target = (int(comment.split(':')[0], 16) + (lit - (1 << 32) if lit >= 1 << 31 else lit))
            if target in at:
                funcs[name][1].add(at[target])
    return kernels, funcs, symbols


def kernels_reaching_lds_users(kernels, funcs):
    """{kernel: a function that is not a kernel, has LDS instructions and is reached from the kernel}"""
    found = {}
    for k in kernels:
        seen, todo = set(), [k]
        while todo:
            for c in funcs.get(todo.pop(), (False, ()))[1]:
                if c not in seen and c not in kernels:
                    seen.add(c); todo.append(c)
        users = sorted(f for f in seen if funcs[f][0])
        if users:
            found[k] = users[0]
    return found


def test_static_lds_of_the_kernels_is_the_constant_and_no_table(tmp_path):
    built = [n for n in LIBS if os.path.exists(os.path.join(PKG, n))]
    assert 'libsrbm_rti.so' in built and 'libsrbm_rti_large.so' in built, 'build() makes both production libraries'
    for n in built:
        base = lds_base(LIBS[n])
        d = tmp_path / n
        d.mkdir()
        checked = 0
        for co in code_objects(os.path.join(PKG, n), str(d)):
            kernels, funcs, symbols = analyse(co)
            if n in KEEPS_TABLE:
                assert TABLE in symbols, (n, 'this build no longer names srbm_lds out of line: take it out of KEEPS_TABLE')
            else:
                assert TABLE not in symbols, (n, 'a function that is not a kernel names srbm_lds: use SRBM_LDS_OUT_OF_LINE()')
            reach = kernels_reaching_lds_users(kernels, funcs)
            for k, user in sorted(reach.items()):
                assert kernels[k] == base, (n, k, 'static LDS %d, SRBM_LDS_BASE %d, reaches %s' % (kernels[k], base, user))
            checked += len(reach)
            fused = [k for k in kernels if 'srbm_rti_fused' in k]
            assert fused and all(k in reach for k in fused), (n, 'the fused kernels call the out-of-line phases')
        print('%s: %d kernels reach an out-of-line LDS user, static LDS %d each' % (n, checked, base))
        assert checked >= 10, (n, checked)


def test_the_check_sees_a_kernel_with_other_static_lds():
    """the rule on a made-up call graph: a kernel with static LDS that reaches an LDS user through a second function is found, one that
    reaches none is not"""
    kernels = {'k_ok': 0, 'k_bad': 8, 'k_free': 4096}
    funcs = {'k_ok': [True, {'f'}], 'k_bad': [False, {'g'}], 'k_free': [True, {'h'}], 'g': [False, {'f', 'h'}], 'f': [True, set()], 'h': [False, set()]}
    reach = kernels_reaching_lds_users(kernels, funcs)
    assert reach == {'k_ok': 'f', 'k_bad': 'f'}
    assert [k for k in reach if kernels[k] != 0] == ['k_bad']
