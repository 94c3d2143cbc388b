"""The binding derived from include/tdr.h (textualdegremoval_amd/_lib.py) against the hand-written one of the parent commit.

Only meant to run at the commit that replaced the hand-written tables.  It loads `git show HEAD~1:textualdegremoval_amd/_lib.py` (or the
revision given as the first argument) from a temporary file and compares ABI_VERSION, SIGNATURES entry by entry (restype, length, every
argtype) and every struct's _fields_ (names, types), ctypes.sizeof and field offsets.  Expected differences: HOST_POINTERS below and the
struct TdrWg1GroupEntry, which the hand-written binding left out; anything else is UNEXPECTED and the exit status is 1.  No GPU.

    python profiles/cabi_binding/compare_with_parent.py [REV] > profiles/cabi_binding/equivalence.txt
"""
import ctypes as C
import importlib.util
import os
import subprocess
import sys
import tempfile

# the host-pointer arguments the hand-written table typed POINTER(T); their callers pass ctypes arrays or byref(), which c_void_p takes too
HOST_POINTERS = {('tdr_tksa_softmax', 4), ('tdr_tksa_bwd', 4), ('tdr_adamw_step', 10), ('tdr_comm_init', 0),
                 ('tdr_wgrad3x3_p16_group_plan', 2), ('tdr_wgrad3x3_p16_group_plan', 3), ('tdr_wgrad3x3_p16_group_plan', 4)}
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def tname(t):
    return f'POINTER({tname(t._type_)})' if hasattr(t, 'contents') else t.__name__


def structs_of(mod):
    return {k: v for k, v in vars(mod).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}


def layout(s):
    return [(n, tname(t), getattr(s, n).offset) for n, t in s._fields_] + [('sizeof', C.sizeof(s))]


def canon(t):
    """an argtype up to the module it came from: each module has its own struct classes, so POINTER(TdrXDesc) compares by layout"""
    return (tname(t), layout(t._type_)) if hasattr(t, 'contents') and issubclass(t._type_, C.Structure) else tname(t)


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else 'HEAD~1'
    src = subprocess.run(['git', 'show', f'{rev}:textualdegremoval_amd/_lib.py'], cwd=ROOT, check=True, capture_output=True, text=True).stdout
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'parent_lib.py')
        with open(path, 'w') as f:
            f.write(src)
        spec = importlib.util.spec_from_file_location('parent_lib', path)
        old = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(old)
    from textualdegremoval_amd import _lib as new

    expected, unexpected = [], []
    print(f'ABI_VERSION parent {old.ABI_VERSION} derived {new.ABI_VERSION}')
    if old.ABI_VERSION != new.ABI_VERSION:
        unexpected.append('ABI_VERSION differs')
    for name in sorted(set(old.SIGNATURES) ^ set(new.SIGNATURES)):
        unexpected.append(f'{name}: only in the {"parent" if name in old.SIGNATURES else "derived"} SIGNATURES')
    same = 0
    for name in sorted(set(old.SIGNATURES) & set(new.SIGNATURES)):
        (ro, ao), (rn, an) = old.SIGNATURES[name], new.SIGNATURES[name]
        diffs = [] if ro is rn else [f'restype {tname(ro)} -> {tname(rn)}']
        if len(ao) != len(an):
            diffs.append(f'{len(ao)} -> {len(an)} arguments')
        for i, (a, b) in enumerate(zip(ao, an)):
            if canon(a) != canon(b):
                host_pointer = (name, i) in HOST_POINTERS and hasattr(a, 'contents') and b is C.c_void_p
                (expected if host_pointer else diffs).append(f'{name} arg {i}: {tname(a)} -> {tname(b)}')
        unexpected += [d if d.startswith(name) else f'{name}: {d}' for d in diffs]
        same += not diffs
    print(f'SIGNATURES parent {len(old.SIGNATURES)} derived {len(new.SIGNATURES)}; {same} entries agree in restype, length and every argtype '
          '(up to the expected differences below)')
    so, sn, agree = structs_of(old), structs_of(new), []
    for name in sorted(set(so) | set(sn)):
        if name not in so:
            (expected if name == 'TdrWg1GroupEntry' else unexpected).append(f'{name}: new struct, sizeof {C.sizeof(sn[name])}')
        elif name not in sn:
            unexpected.append(f'{name}: struct missing from the derived binding')
        elif layout(so[name]) != layout(sn[name]):
            unexpected.append(f'{name}: layout differs: {[p for p in zip(layout(so[name]), layout(sn[name])) if p[0] != p[1]][:3]}')
        else:
            agree.append(f'{name} {len(sn[name]._fields_)} / {C.sizeof(sn[name])}')
    print(f'{len(agree)} structs agree in field names, types, offsets and sizeof (fields / bytes): ' + ', '.join(agree))
    print('\n  '.join([f'expected differences ({len(expected)}):'] + expected))
    print('\n  '.join([f'UNEXPECTED differences ({len(unexpected)}):'] + unexpected))
    return 1 if unexpected else 0


if __name__ == '__main__':
    sys.exit(main())
