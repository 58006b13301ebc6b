"""The Karel program-metrics launch (include/d2p.h d2p_karel_exec, csrc/karel_exec.hip) on the CPU side: declared in
the header and the ctypes table with the same arity, its workspace query answers without a GPU (0 for geometries the
launch does not take), and bad arguments return D2P_EINVAL before anything reaches the GPU."""
import os
import re

from demo2program_amd import lib as d2plib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('d2p_karel_exec_ws_bytes', 'd2p_karel_exec')


def _prototypes():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'd2p.h')).read(), flags=re.S)
    out = {}
    for m in re.finditer(r'\b(?:int|size_t)\s+(d2p_karel_exec\w*)\s*\(([^;]*?)\)\s*;', src, flags=re.S):
        out[m.group(1)] = len([a for a in m.group(2).split(',') if a.strip()])
    return out


def test_entry_points_are_declared_with_matching_arity():
    protos = _prototypes()
    assert set(protos) == set(NAMES)
    for name in NAMES:
        assert len(d2plib.SIGNATURES[name][1]) == protos[name], name
    assert protos['d2p_karel_exec'] == 31
    src = open(os.path.join(ROOT, 'demo2program_amd', 'build.py')).read()
    assert "'karel_exec.hip'" in src


def test_workspace_query_needs_no_gpu(d2p_lib):
    ws = d2p_lib.d2p_karel_exec_ws_bytes
    assert ws(32, 45, 8, 8, 16) >= 32 * 4
    assert ws(1, 128, 4, 16, 16) > 0 and ws(7, 1, 1, 1, 16) > 0
    # geometries the launch does not take: the caller uses the host path
    for args in ((0, 45, 8, 8, 16), (32, 0, 8, 8, 16), (32, 129, 8, 8, 16), (32, 45, 9, 8, 16),
                 (32, 45, 8, 8, 15), (32, 45, 8, 8, 17), (32, 45, 0, 8, 16)):
        assert ws(*args) == 0, args


def _launch(lib, B=2, L=8, h=8, w=8, depth=16, flags=0, k=3, T=4, frames=1, cs=16, dlen=1, k2=0, T2=0,
            frames2=None, cs2=0, dlen2=None, outs=1, execution=None, T_out=0, ws=1, ws_bytes=None):
    """Every pointer is a fake non-null HOST address: the call must return before a pointer is dereferenced."""
    p = 0x1000 if outs else None
    if ws_bytes is None:
        ws_bytes = lib.d2p_karel_exec_ws_bytes(B, L, h, w, depth)
    return lib.d2p_karel_exec(B, L, p or 0x1000, L, 0x1000, 0x1000, h, w, depth, flags,
                              k, T, 0x1000 if frames else None, cs, 0x1000 if dlen else None,
                              k2, T2, 0x1000 if frames2 else None, cs2, 0x1000 if dlen2 else None,
                              p, p, p, p, None, None, execution, T_out, 0x1000 if ws else None, ws_bytes, None)


def test_argument_errors_return_einval_without_a_gpu(d2p_lib):
    bad = [dict(B=0), dict(B=-3), dict(L=0), dict(L=129), dict(depth=15), dict(h=9), dict(w=0),
           dict(k=0), dict(k=-1), dict(T=0), dict(frames=0), dict(dlen=0), dict(cs=15),
           dict(k2=2, T2=4, frames2=1, cs2=16, dlen2=None), dict(k2=2, T2=0, frames2=1, cs2=16, dlen2=1),
           dict(k2=2, T2=4, frames2=None, cs2=16, dlen2=1), dict(outs=0), dict(T_out=5), dict(T_out=-1),
           dict(ws=0), dict(ws_bytes=1), dict(flags=16)]
    for kw in bad:
        assert _launch(d2p_lib, **kw) == -1, kw
        assert d2p_lib.d2p_last_error().startswith(b'karel_exec'), kw
    msg = (_launch(d2p_lib, h=9) and d2p_lib.d2p_last_error()).decode()
    assert 'unsupported geometry' in msg


def test_the_host_path_switch_is_declared():
    from demo2program_amd import options
    default, _, test = options.SWITCHES['D2P_HOST_PROGRAM_METRICS']
    assert default == '0' and test.startswith('tests/test_karel_exec_gpu.py::')


def test_ld_tok_below_L_is_refused(d2p_lib):
    L = 8
    rc = d2p_lib.d2p_karel_exec(2, L, 0x1000, L - 1, 0x1000, 0x1000, 8, 8, 16, 0, 3, 4, 0x1000, 16, 0x1000,
                                0, 0, None, 0, None, 0x1000, 0x1000, 0x1000, 0x1000, None, None, None, 0,
                                0x1000, d2p_lib.d2p_karel_exec_ws_bytes(2, L, 8, 8, 16), None)
    assert rc == -1
