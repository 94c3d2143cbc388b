"""Host-side checks of the fused TLSC path (no GPU): tdr_naf_tail_infer_local is declared, bound and exported, the ABI constant moved
with it, its argument checks run before anything is launched, and the engine has its module switch."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = 'tdr_naf_tail_infer_local'


def test_header_binding_and_library_agree_on_the_entry():
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, 'include', 'tdr.h')).read()
    assert re.search(r'^int ' + SYMBOL + r'\(const TdrNafTailLocalDesc\* d, void\* stream\);', txt, re.M), 'not declared in include/tdr.h'
    assert SYMBOL in _lib.SIGNATURES and hasattr(lib, SYMBOL), 'not bound / not exported by the built library'
    assert int(re.search(r'#define TDR_ABI_VERSION (\d+)', txt).group(1)) == _lib.ABI_VERSION == lib.tdr_version() == 112
    # the descriptor: the header's fields in the header's order; TdrNafTailDesc without saved tensors, c_out and the sca row
    body = re.search(r'typedef struct TdrNafTailLocalDesc \{(.*?)\} TdrNafTailLocalDesc;', txt, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [t for t in re.findall(r'\w+', body) if t not in ('int', 'float', 'const', 'void', 'int64_t')]
    assert names == [n for n, _ in _lib.TdrNafTailLocalDesc._fields_]
    plain = [n for n, _ in _lib.TdrNafTailDesc._fields_]
    local = [n for n, _ in _lib.TdrNafTailLocalDesc._fields_]
    assert not set(local) & {'y', 'mu', 'rs', 'yn', 't4', 'c_out', 'sca'} and set(local) - set(plain) == {'pool', 'pool_ns', 'wsca', 'bsca'}


def test_entry_checks_its_arguments_before_any_launch():
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    fn, desc = lib.tdr_naf_tail_infer_local, _lib.TdrNafTailLocalDesc

    def filled(skip=()):
        d = desc()
        for name, typ in desc._fields_:
            if typ is C.c_void_p and name not in skip:
                setattr(d, name, 64)
        d.N, d.C, d.HW, d.w_fmt = 1, 32, 64, 1
        return d
    for missing in ('pool', 'wsca', 'bsca', 'out'):
        assert fn(C.byref(filled([missing])), None) != 0 and 'null pointer' in lib.tdr_last_error().decode(), missing
    for c, hw in ((48, 64), (512, 64), (64, 96)):                    # the support predicate is tdr_naf_tail_supported's
        d = filled()
        d.C, d.HW = c, hw
        assert not lib.tdr_naf_tail_supported(c, hw)
        assert fn(C.byref(d), None) != 0 and 'needs C in {32, 64, 128, 256}' in lib.tdr_last_error().decode(), (c, hw)
    d = filled()
    d.w_fmt = 0
    assert fn(C.byref(d), None) != 0 and 'must be packed' in lib.tdr_last_error().decode()


def test_engine_switch_and_wrapper():
    from textualdegremoval_amd import engine as E, kernels as K
    assert E.LOCAL_KERNELS is True                                   # module switch (A/B in profiles/probe_tlsc_infer.py), no environment knob
    assert list(inspect.signature(K.naf_tail_infer_local).parameters) == [
        'g', 'pooled', 'x', 'wscap', 'bsca', 'w3p', 'b3', 'beta', 'lnw', 'lnb', 'eps', 'w4p', 'b4', 'w5p', 'b5', 'gamma']
    assert list(inspect.signature(E.naf_fwd_local).parameters) == ['x', 'P', 'k1', 'k2']
