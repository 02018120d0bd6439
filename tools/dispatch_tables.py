"""Host-side dispatch table of one libfwn.so build, for diffing two builds (CPU only: nothing runs on a GPU).

    python tools/dispatch_tables.py LIB OUT

Writes fwn_workspace_bytes / fwn_train_workspace_bytes and the four ragged workspace queries (fwn_ragged_workspace_bytes,
fwn_ragged_forward_workspace_bytes, fwn_ragged_init_workspace_bytes, fwn_train_ragged_workspace_bytes) over BASELINE-like and
small configs (B 1 - 16, several T, every cond_mode / persist_mode / chain_mode, with and without tail / conditioning streams
and the fp8 gate), the per-block
fwn_flow_persist_supported / fwn_cond_stream_splits, and the four tail queries plus the split counts over M = 1 .. 2^17.
Descriptors carry dummy aligned weight pointers: the host never dereferences them.  A change to host dispatch that must
not change what runs keeps the table identical:  python tools/dispatch_tables.py <old lib> a.txt; ... <new lib> b.txt;
cmp a.txt b.txt"""
import ctypes as C
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_flowavenet_amd import _lib as L_
lib = C.CDLL(sys.argv[1])
out = open(sys.argv[2], "w")
FD, MD, TD, FTD = L_.FlowDesc, L_.ModelDesc, L_.TrainDesc, L_.FlowTrainDesc
lib.fwn_workspace_bytes.restype = C.c_size_t
lib.fwn_workspace_bytes.argtypes = [C.POINTER(MD), C.c_int64, C.c_int64]
lib.fwn_train_workspace_bytes.restype = C.c_size_t
lib.fwn_train_workspace_bytes.argtypes = [C.POINTER(TD), C.c_int64, C.c_int64]
RAGGED = ("fwn_ragged_workspace_bytes", "fwn_ragged_forward_workspace_bytes", "fwn_ragged_init_workspace_bytes")
for q in RAGGED:
    getattr(lib, q).restype = C.c_size_t
    getattr(lib, q).argtypes = [C.POINTER(MD), C.c_int64, C.c_int64]
lib.fwn_train_ragged_workspace_bytes.restype = C.c_size_t
lib.fwn_train_ragged_workspace_bytes.argtypes = [C.POINTER(TD), C.c_int64, C.c_int64]
lib.fwn_flow_persist_supported.argtypes = [C.POINTER(FD), C.c_int64, C.c_int64]
FAKE = [0x7f0000000000]
def fp():
    FAKE[0] += 0x100000
    return FAKE[0]
def roundup(a, b): return (a + b - 1) // b * b
def flow(ch, L, cin, wts):
    d = FD()
    kcpad, kfpad, npt = roundup(cin, 64), roundup(3 * ch, 64), max(1, (ch + 31) // 32)
    d.Ch, d.cin, d.kcpad, d.kfpad, d.npt, d.L = ch, cin, kcpad, kfpad, npt, L
    d.Wfront = fp(); d.bfront = fp()
    for l in range(L):
        d.Wd[l] = fp(); d.Wc[l] = fp(); d.bgate[l] = fp(); d.Wres[l] = fp(); d.bres[l] = fp()
    d.Wskip = fp(); d.bskip = fp(); d.Wfinal = fp(); d.bfinal = fp(); d.Wzero = fp(); d.bzero = fp(); d.ezero = fp(); d.an = fp()
    if ch >= 16: d.Wfront2 = fp()
    if ch <= 8: d.Wfront3 = fp(); d.kf3 = roundup(6 * ch, 16)
    if wts and npt == 1 and L == 2: d.Wts = fp()
    return d
def model(nb, nf, L, mels, ups, cm, pm, chm, wts, cs, fp8):
    flows = (FD * (nb * nf))()
    for i in range(nb):
        for j in range(nf):
            flows[i * nf + j] = flow(1 << i, L, (mels // 2) * (2 << i), wts)
    m = MD()
    m.n_block, m.n_flow, m.n_layer, m.num_mels, m.n_up = nb, nf, L, mels, len(ups)
    for k, s in enumerate(ups): m.up_scale[k] = s; m.up_w[k] = fp()
    m.flows = flows; m.cond_mode, m.persist_mode, m.chain_mode, m.gate_fp8 = cm, pm, chm, fp8
    if cs:
        for i in range(nb): m.cond_stream[i] = fp()
    m._keep = flows
    return m
def tdesc(m):
    t = TD(); t.model = C.pointer(m)
    ft = (FTD * (m.n_block * m.n_flow))(); t.flows = ft; t._keep = ft
    for i in range(m.n_block):
        for a in ("cond_rows", "front_rows", "zinv32", "br", "zcol"): getattr(t, a)[i] = fp()
    for k in range(m.n_up): t.up_bias_dev[k] = fp()
    return t
cfgs = [("c1", 8, 6, 2, 80, [16, 16], [1, 2, 3, 8, 16], [16000, 16128, 6400, 220672, 4096]),
        ("c0", 2, 2, 2, 80, [16, 16], [1, 2, 3, 8, 16], [16128, 6400, 4096]),
        ("k8", 5, 6, 2, 80, [8, 12], [1, 2, 3, 8, 16], [2304, 16128, 96 * 64]),
        ("small", 3, 2, 2, 16, [4, 4], [1, 2, 3, 8, 16], [256, 512, 1024]),
        ("small3", 2, 2, 3, 8, [4, 4], [1, 2, 3, 8, 16], [256, 1024])]
for (name, nb, nf, L, mels, ups, Bs, Ts) in cfgs:
    for cm, pm, chm, wts, cs, fp8 in itertools.product([0, 1, 2], [0, 1, 2], [0, 1], [0, 1], [0, 1], [0, 1]):
        m = model(nb, nf, L, mels, ups, cm, pm, chm, wts, cs, fp8)
        t = tdesc(m)
        for B in Bs:
            for T in Ts:
                ws = lib.fwn_workspace_bytes(C.byref(m), B, T)
                tw = lib.fwn_train_workspace_bytes(C.byref(t), B, T) if (cm, pm, chm, cs, fp8) == (0, 0, 0, 0, 0) else -1
                out.write("ws %s cm%d pm%d ch%d wts%d cs%d fp8%d B%d T%d %d %d\n" % (name, cm, pm, chm, wts, cs, fp8, B, T, ws, tw))
                # the ragged queries on the same rows (the training one where the training query is asked)
                rw = [getattr(lib, q)(C.byref(m), B, T) for q in RAGGED]
                rt = lib.fwn_train_ragged_workspace_bytes(C.byref(t), B, T) if tw != -1 else -1
                out.write("rws %s cm%d pm%d ch%d wts%d cs%d fp8%d B%d T%d %d %d %d %d\n" % (name, cm, pm, chm, wts, cs, fp8, B, T, *rw, rt))
                if (cm, pm, chm, cs, fp8) == (0, 0, 0, 0, 0):
                    for i in range(nb):
                        d = m.flows[i * nf]
                        M = B * T // (2 << i)
                        out.write("q %s wts%d B%d T%d blk%d persist %d cstream %d\n" % (name, wts, B, T, i,
                                  lib.fwn_flow_persist_supported(C.byref(d), B, T), lib.fwn_cond_stream_splits(M, nf * L, d.kcpad)))
# tail queries over a sweep of M
Ms = sorted(set([1, 2, 3, 63, 64, 65] + [int(round(2 ** (e / 8.0))) for e in range(0, 8 * 17 + 1)] +
               [1007, 1008, 1009, 6143, 6144, 6145, 12287, 12288, 12289, 49151, 49152, 49153, 4095, 4096, 4097, 131072]))
for ch in [1, 2, 4, 8, 16, 32, 64, 128]:
    for L in [1, 2, 3]:
        for wts in [0, 1]:
            d = flow(ch, L, 80 * ch, wts)
            for M in Ms:
                out.write("t ch%d L%d wts%d M%d %d %d %d %d %d %d %d %d %d %d\n" % (ch, L, wts, M, lib.fwn_tail_partials(M),
                          lib.fwn_tail_partials_chained(M, ch, 0), lib.fwn_tail_partials_chained(M, ch, 1),
                          lib.fwn_tail_partials_desc(C.byref(d), M, -1), lib.fwn_tail_partials_desc(C.byref(d), M, 0),
                          lib.fwn_tail_partials_desc(C.byref(d), M, 1), lib.fwn_tail_can_chain(C.byref(d), M, 0),
                          lib.fwn_tail_can_chain(C.byref(d), M, 1), lib.fwn_cond_stream_splits(M, 12, d.kcpad),
                          lib.fwn_cond_splits(M, 6, d.kcpad)))
out.close()
