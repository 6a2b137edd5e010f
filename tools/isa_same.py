"""Are kernels the code they were?  Compares every kernel whose name contains one of the patterns
in two sets of -save-temps ISA files (`make asm` keeps them): the instruction streams,
instruction by instruction with block labels renumbered and comments dropped, and the kernel
descriptors' `.amdhsa_*` values (VGPR and SGPR counts, LDS and scratch sizes, accum offset, ...):

    python tools/isa_same.py BEFORE.s AFTER.s ref_sweep_kernel ref_chain [--drop-arg ', false>']
    python tools/isa_same.py BEFORE.s : AFTER1.s AFTER2.s ... _kernel

Either side may be several files (a side's kernels are the union of its files', and a kernel
found in more than one file of a side, a template compiled in two units, is reported); a `:`
then separates BEFORE's files from AFTER's.  --drop-arg removes a trailing template argument from
AFTER's demangled names before matching (a template flag added with a default); kernels only
AFTER has are listed as new.  Exit status 1 if a kernel both sides have differs or is missing,
or a side has a kernel twice.
"""
import argparse
import re
import subprocess
import sys


def kernels(paths, patterns):
    """{demangled name: (instructions, {.amdhsa_ field: value})} over the files, and the mangled
    names found in more than one of them (the last file's text is the one kept)"""
    code, desc, cur, twice = {}, {}, None, []
    for path in paths:
        dcur = None
        for line in open(path):
            m = re.match(r'^(_Z\w+):', line)
            if m:
                cur = m.group(1) if any(p in m.group(1) for p in patterns) else None
                if cur:
                    if cur in code:
                        twice.append(f'{cur} (again in {path})')
                    code[cur] = []
                continue
            m = re.match(r'^\s+\.amdhsa_kernel\s+(\S+)', line)
            if m:
                dcur = desc.setdefault(m.group(1), {})
                continue
            if dcur is not None:
                m = re.match(r'^\s+(\.amdhsa_\w+)\s+(\S+)', line)
                if m:
                    dcur[m.group(1)] = m.group(2)
                elif '.end_amdhsa_kernel' in line:
                    dcur = None
                continue
            if cur is None:
                continue
            if line.startswith('.Lfunc_end'):
                cur = None
                continue
            text = re.sub(r';.*', '', re.sub(r'\.LBB\d+_', '.LBB_', line)).rstrip()
            if text and (not text.lstrip().startswith('.') or text.startswith('.LBB')):
                code[cur].append(text)
    names = subprocess.run(['c++filt'], input='\n'.join(code), capture_output=True, text=True).stdout.split('\n')
    return {n.replace('kfmi::(anonymous namespace)::', ''): (code[k], desc.get(k, {})) for n, k in zip(names, code)}, twice


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('args', nargs='+', metavar='ARG', help='BEFORE.s ... [:] AFTER.s ... PATTERN ...')
    ap.add_argument('--drop-arg', default=None)
    args = ap.parse_args()
    files = [x for x in args.args if x.endswith('.s') or x == ':']
    patterns = args.args[len(files):]
    if args.args[:len(files)] != files or not patterns:
        ap.error('the .s files come first, then at least one pattern')
    if ':' in files:
        before, after = files[:files.index(':')], files[files.index(':') + 1:]
    else:
        before, after = files[:1], files[1:]
    if not before or not after or ':' in after or (':' not in files and len(files) != 2):
        ap.error('BEFORE.s AFTER.s, or BEFORE.s ... : AFTER.s ...')
    (a, twice_a), (b, twice_b) = kernels(before, patterns), kernels(after, patterns)
    if args.drop_arg:
        b = {(k.replace(args.drop_arg, '>', 1) if k.replace(args.drop_arg, '>', 1) in a else k): v for k, v in b.items()}
    same = bad = 0
    for side, twice in (('before', twice_a), ('after', twice_b)):
        for k in twice:
            print(f'in two files {side}: {k}')
            bad += 1
    for k, (code, desc) in a.items():
        if k not in b:
            print('missing after:', k)
            bad += 1
        elif code != b[k][0]:
            print(f'differs: {k} ({len(code)} -> {len(b[k][0])} instructions)')
            bad += 1
        elif not desc or not b[k][1]:
            print('no descriptor found:', k)
            bad += 1
        elif desc != b[k][1]:
            fields = sorted(f for f in set(desc) | set(b[k][1]) if desc.get(f) != b[k][1].get(f))
            print(f'descriptor differs: {k}: ' + ', '.join(f'{f} {desc.get(f)} -> {b[k][1].get(f)}' for f in fields))
            bad += 1
        else:
            same += 1
    for k in b:
        if k not in a:
            print(f'new: {k} ({len(b[k][0])} instructions)')
    print(f'{same} kernels the same, {bad} not, of {len(a)} before and {len(b)} after')
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
