"""Compare the compiled kernels of two source trees, kernel by kernel: the instruction text
(comments, directives and debug lines stripped; the function index of local labels normalised)
and the kernel descriptor values (register, spill, LDS and scratch sizes).  For refactors that
must not change what runs on the GPU.  Kernels are matched by base name plus all their template
arguments; every selected source of each tree (--sources, a glob within csrc; default the split
block sources block_*_split*.hip) is compiled with the project's flags for that source
(_build.FLAGS + EXTRA.get(name, []), --cuda-device-only -S).

usage: python tools/diag/isa_compare.py <old csrc dir> <new csrc dir> [--sources GLOB] [--keep DIR]
--keep DIR leaves the listings in DIR/old and DIR/new; a directory of such listings may stand in
for a csrc directory.  Exit status 0 when every kernel compares equal"""
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from audio_style_transfer_amd import _build  # noqa: E402

DESC = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.sgpr_spill_count', '.vgpr_spill_count',
        '.group_segment_fixed_size', '.private_segment_fixed_size')
SOURCES = 'block_*_split*.hip'


def compile_tree(csrc, out, sources=SOURCES):
    srcs = sorted(glob.glob(os.path.join(csrc, sources)))
    if not srcs:   # a directory of listings kept from an earlier run
        return sorted(glob.glob(os.path.join(csrc, os.path.splitext(sources)[0] + '.s')))

    def cc(src):
        s = os.path.join(out, os.path.basename(src)[:-4] + '.s')
        cmd = [_build.HIPCC, *_build.FLAGS, '-I', csrc, *_build.EXTRA.get(os.path.basename(src), []),
               '--cuda-device-only', '-S', src, '-o', s]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError('hipcc failed for %s:\n%s' % (src, r.stderr))
        return s

    with ThreadPoolExecutor(len(srcs)) as ex:
        return list(ex.map(cc, srcs))


def demangle(names):
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def key_of(demangled):
    """'k_block_fwd_s16<true,false,false>' / 'k_gram_fwd_n<2,4>' from the kernel's demangled name"""
    m = re.search(r'(\w+)(?:<(.*?)>)?\(', demangled)
    args = re.sub(r'\s+', '', m.group(2) or '')
    return m.group(1) + ('<%s>' % args if args else '')


def kernels(path):
    """{mangled name: (instruction lines, {descriptor field: value})} of one listing"""
    body, name, text, meta, cur, funcs = {}, None, [], {}, None, set()
    for l in open(path).read().splitlines():
        m = re.match(r'^\s*\.type\s+(\w+),@function', l)
        if m:
            funcs.add(m.group(1))
        m = re.match(r'^(\w+):', l)
        if m and name is None and m.group(1) in funcs:
            name, text = m.group(1), []
            continue
        if name is not None:
            if l.startswith('.Lfunc_end'):
                body[name], name = text, None
                continue
            s = l.split(';')[0].split('//')[0].strip()
            if not s or (s.startswith('.') and not s.endswith(':')):
                continue   # comment, directive or debug line
            text.append(re.sub(r'\.L(BB|tmp)\d+', r'.L\1#', s))
            continue
        m = re.match(r'^  - (\.\w+):\s*(\S+)', l)
        if m:   # a new kernel entry of amdhsa.kernels
            cur = {}
        m = re.match(r'^  [ -] (\.\w+):\s*(\S+)\s*$', l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == '.name':
                meta[m.group(2)] = cur
    return {n: (t, {f: meta.get(n, {}).get(f) for f in DESC}) for n, t in body.items() if n in meta}


def tree_kernels(listings):
    out = {}
    for s in listings:
        ks = kernels(s)
        dm = demangle(list(ks))
        for n, v in ks.items():
            k = key_of(dm[n]) if n.startswith('_Z') else n
            assert k not in out, 'two kernels named ' + k
            out[k] = v
    return out


def main():
    keep = sys.argv[sys.argv.index('--keep') + 1] if '--keep' in sys.argv else None
    sources = sys.argv[sys.argv.index('--sources') + 1] if '--sources' in sys.argv else SOURCES
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as tmp:
        root = keep or tmp
        trees = []
        for tag, d in (('old', old_dir), ('new', new_dir)):
            out = os.path.join(root, tag)
            os.makedirs(out, exist_ok=True)
            trees.append(tree_kernels(compile_tree(d, out, sources)))
    old, new = trees
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            print('%-50s only in %s' % (k, 'old' if k in old else 'new'))
            bad += 1
            continue
        (to, do), (tn, dn) = old[k], new[k]
        nd = sum(1 for l in difflib.unified_diff(to, tn, lineterm='', n=0)
                 if l[:1] in '+-' and l[:3] not in ('+++', '---')) if to != tn else 0
        dd = {f: (do[f], dn[f]) for f in DESC if do[f] != dn[f]}
        if nd or dd:
            bad += 1
        print('%-50s %6d lines  %s' % (k, len(tn), 'equal' if not nd and not dd else
                                      '%d differing lines %s' % (nd, dd or '')))
    print('%d kernels compared, %d differ' % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
