#!/usr/bin/env python3
"""Registers, spills, scratch and LDS of every kernel of a gfx950 code object, from its metadata notes (no GPU needed).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include --cuda-device-only -c gan-control_amd/csrc/conv_bf16x3.hip -o /tmp/x.bundle
    python tools/kernel_regs.py /tmp/x.bundle [--all]        # default: only kernels that spill or use scratch
    python tools/kernel_regs.py --digest /tmp/*.bundle       # one line per kernel: name, hash of its instruction text, the same metadata

--digest is the instrument of a refactor that must not change device code: run it over every unit before and after (both
arithmetics) and compare the lines by kernel name (the table is sorted by name, so `diff` does it).  The hash covers the
disassembly of the kernel's symbol with the trailing `// address: encoding` comments stripped; branch targets are
kernel-relative there, so a kernel keeps its hash when it moves to another unit or another offset.
"""
import hashlib
import re
import subprocess
import sys
import tempfile

LLVM = '/opt/rocm/lib/llvm/bin/'


def code_object(path):
    dev = tempfile.mktemp(suffix='.co')
    r = subprocess.run([LLVM + 'clang-offload-bundler', '--unbundle', '--type=o', '--input=' + path, '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + dev],
                       capture_output=True, text=True)
    return dev if r.returncode == 0 else path       # else: already a bare code object


def demangle(names):
    out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return dict(zip(names, out))


def kernels(dev):
    """[(mangled name, metadata getter)] of a code object"""
    txt = subprocess.run([LLVM + 'llvm-readelf', '--notes', dev], capture_output=True, text=True, check=True).stdout
    res = []
    for k in re.split(r'\n\s+- \.agpr_count', txt)[1:]:
        g = lambda key, k=k: (re.search(r'\.' + key + r':\s+(\S+)', k) or [None, None])[1]
        res.append((g('name'), g))
    return res


def isa_hashes(dev):
    """mangled symbol -> sha256 (16 hex digits) of its instruction text"""
    txt = subprocess.run([LLVM + 'llvm-objdump', '-d', '--no-show-raw-insn', '--no-leading-addr', dev], capture_output=True, text=True, check=True).stdout
    res, cur, h = {}, None, None
    for line in txt.split('\n'):
        m = re.match(r'^(?:[0-9a-f]+ )?<([^>]+)>:$', line)
        if m:
            # basic-block labels (<L123>, <.LBB...>) belong to the kernel they sit in
            if re.match(r'^(L\d+|\.L)', m.group(1)) and cur:
                h.update(b'label\n')
                continue
            if cur:
                res[cur] = h.hexdigest()[:16]
            cur, h = m.group(1), hashlib.sha256()
            continue
        if cur and line.strip() and line.strip() != '...':          # (`...`: the zero padding behind a kernel, which depends on what follows it)
            h.update((re.sub(r'\s*//.*$', '', line).strip() + '\n').encode())
    if cur:
        res[cur] = h.hexdigest()[:16]
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    show_all, digest = '--all' in sys.argv, '--digest' in sys.argv
    rows = []
    for path in args:
        dev = code_object(path)
        ks = kernels(dev)
        names = demangle([n for n, _ in ks])
        isa = isa_hashes(dev) if digest else {}
        for mangled, g in ks:
            full = re.sub(r'\(anonymous namespace\)::', '', names[mangled])
            meta = 'vgpr %3s  vgpr_spill %3s  sgpr %3s  sgpr_spill %3s  scratch %4s B  lds %6s B' % (
                g('vgpr_count'), g('vgpr_spill_count'), g('sgpr_count'), g('sgpr_spill_count'), g('private_segment_fixed_size'), g('group_segment_fixed_size'))
            if digest:
                # the full template arguments: instances of one kernel must stay apart (the argument list of the call is dropped)
                rows.append('%s  %s  %s' % (isa[mangled], meta, re.sub(r'\((?:[^()]|\([^()]*\))*\)$', '', full)))
                continue
            spill = int(g('vgpr_spill_count') or 0) + int(g('sgpr_spill_count') or 0) + int(g('private_segment_fixed_size') or 0)
            if show_all or spill:
                print('%-64s %s' % (full.split('(')[0][:64], meta))
    for r in sorted(rows, key=lambda r: r.split('  ')[-1]):
        print(r)


if __name__ == '__main__':
    main()
