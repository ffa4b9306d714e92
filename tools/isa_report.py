#!/usr/bin/env python3
"""Per-kernel resource table of the HIP engine as built by THIS toolchain.

    python tools/isa_report.py            print the table
    python tools/isa_report.py --write    ... and rewrite profiles/r07_isa_resources.txt (tests/test_isa.py prints a warning when a build differs)
    python tools/isa_report.py --source F  ... of the kernel source F (a copy of an earlier cw_kernels.hip, say) instead of the tree's

Source: hipcc -Rpass-analysis=kernel-resource-usage (registers, spills, scratch, occupancy, LDS) and the -S output of the same run: per function the number
of instructions and a short hash of the instruction stream, so that "this change left that kernel's code as it was" is two equal fields.  The stream is
NORMALISED before it is counted and hashed: directives, comments and blank lines are dropped, and local labels are renumbered in their order of appearance
(a label's number counts the functions and blocks in front of it, which another kernel's change moves)."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gym_craftingworld_amd', 'csrc')
RECORD = os.path.join(ROOT, 'profiles', 'r07_isa_resources.txt')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '--cuda-device-only', '-x', 'hip']


def demangle(names):
    """_Z23cw_render_pieces_kernelILi0ELi2EEv8CwParamsPhiiiii -> cw_render_pieces_kernel<0,2> (Itanium names of plain / int- and bool-templated functions)"""
    out = []
    for n in names:
        m = re.match(r'_Z(\d+)', n)
        if not m:
            out.append(n)
            continue
        k = int(m.group(1))
        base, rest = n[m.end():m.end() + k], n[m.end() + k:]
        t = re.match(r'I((?:L[ib]\d+E)+)E', rest)
        out.append(base + ('<%s>' % ','.join(re.findall(r'L[ib](\d+)E', t.group(1))) if t else ''))
    return out


def streams(asm):
    """{function: (instructions, hash)} of an AMDGPU assembly listing"""
    funcs = set(re.findall(r'^\s*\.type\s+(\S+),@function', asm, re.M))
    out, name, body = {}, None, []
    for line in asm.split('\n'):
        line = line.split(';')[0].rstrip()
        m = re.match(r'(\S+):$', line)
        if name is None:
            if m and m.group(1) in funcs:
                name, body = m.group(1), []
        elif m and m.group(1).startswith('.Lfunc_end'):
            labels = {}
            text = '\n'.join(re.sub(r'\.L\w+', lambda t: labels.setdefault(t.group(0), 'L%d' % len(labels)), l) for l in body)
            out[name] = (sum(1 for l in body if not l.endswith(':')), hashlib.sha256(text.encode()).hexdigest()[:12])
            name = None
        elif line.strip() and not line.strip().startswith('.') or m:
            body.append(' '.join(line.split()))
    return out


def resources(tmp, source):
    r = subprocess.run([HIPCC] + FLAGS + ['-I', CSRC, '-S', '-o', os.path.join(tmp, 'k.s'), source,
                        '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True, check=True)
    with open(os.path.join(tmp, 'k.s')) as f:
        code = streams(f.read())
    rows, cur = [], None
    for line in r.stderr.split('\n'):
        m = re.search(r'remark: +Function Name: (\S+)', line)
        if m:
            cur = {'name': m.group(1)}
            rows.append(cur)
            continue
        m = re.search(r'remark: +([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass', line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    for row in rows:
        row['insts'], row['hash'] = code.pop(row['name'], ('?', '?'))
    return rows, code


def report(source=os.path.join(CSRC, 'cw_kernels.hip')):
    with tempfile.TemporaryDirectory() as tmp:
        rows, device_functions = resources(tmp, source)
    names = demangle([r['name'] for r in rows])
    lines = ['# built by tools/isa_report.py (hipcc -O3 --offload-arch=gfx950); tests/test_isa.py warns when a build differs from this table',
             '%-44s %5s %5s %11s %11s %8s %5s %6s %6s %12s' % ('kernel', 'VGPR', 'SGPR', 'SGPR spills', 'VGPR spills', 'scratch', 'occ', 'LDS', 'insts',
                                                                'hash')]
    for r, n in sorted(zip(rows, names), key=lambda t: t[1]):
        lines.append('%-44s %5s %5s %11s %11s %8s %5s %6s %6s %12s' % (n, r.get('VGPRs', '?'), r.get('TotalSGPRs', '?'), r.get('SGPRs Spill', '?'),
                                                                       r.get('VGPRs Spill', '?'), r.get('ScratchSize', '?'), r.get('Occupancy', '?'),
                                                                       r.get('LDS Size', '?'), r['insts'], r['hash']))
    # (a device function that is called, not inlined, has code but no resource remark of its own: its count and hash only, as a comment)
    for n, (insts, digest) in sorted(zip(demangle(device_functions), device_functions.values())):
        lines.append('# device function %-28s %68s %6s %12s' % (n, '', insts, digest))
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    text = report(sys.argv[sys.argv.index('--source') + 1]) if '--source' in sys.argv else report()
    sys.stdout.write(text)
    if '--write' in sys.argv:
        with open(RECORD, 'w') as f:
            f.write(text)
