"""Are kernels the code they were?  Compares the instruction streams of every kernel whose name
contains one of the patterns in two -save-temps ISA files (`make asm` keeps them), instruction by
instruction with block labels renumbered and comments dropped:

    python tools/isa_same.py BEFORE.s AFTER.s ref_sweep_kernel ref_chain [--drop-arg ', false>']

--drop-arg removes a trailing template argument from AFTER's demangled names before matching (a
template flag added with a default); kernels only AFTER has are listed as new.  Exit status 1 if
a kernel both files have differs or is missing.
"""
import argparse
import re
import subprocess
import sys


def kernels(path, patterns):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r'^(_Z\w+):', line)
        if m:
            cur = m.group(1) if any(p in m.group(1) for p in patterns) else None
            if cur:
                out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
            continue
        text = re.sub(r';.*', '', re.sub(r'\.LBB\d+_', '.LBB_', line)).rstrip()
        if text and (not text.lstrip().startswith('.') or text.startswith('.LBB')):
            out[cur].append(text)
    names = subprocess.run(['c++filt'], input='\n'.join(out), capture_output=True, text=True).stdout.split('\n')
    return {n.replace('kfmi::(anonymous namespace)::', ''): v for n, v in zip(names, out.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('before')
    ap.add_argument('after')
    ap.add_argument('patterns', nargs='+')
    ap.add_argument('--drop-arg', default=None)
    args = ap.parse_args()
    a, b = kernels(args.before, args.patterns), kernels(args.after, args.patterns)
    if args.drop_arg:
        b = {(k.replace(args.drop_arg, '>', 1) if k.replace(args.drop_arg, '>', 1) in a else k): v for k, v in b.items()}
    same = bad = 0
    for k, v in a.items():
        if k not in b:
            print('missing after:', k)
            bad += 1
        elif v != b[k]:
            print(f'differs: {k} ({len(v)} -> {len(b[k])} instructions)')
            bad += 1
        else:
            same += 1
    for k in b:
        if k not in a:
            print(f'new: {k} ({len(b[k])} instructions)')
    print(f'{same} kernels the same, {bad} not, of {len(a)} before and {len(b)} after')
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
