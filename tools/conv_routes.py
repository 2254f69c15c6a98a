#!/usr/bin/env python
"""Everything the host side of the conv family answers about a descriptor, one line per (descriptor, operand layout,
pass): kernel name, executed fraction, workspace bytes, scratch flag, kept-copy layout, and per descriptor the pitch,
statistics, fan-in and kept-transform queries.  CPU only.  Two builds answer the same iff their outputs are equal:
    DCFP_LIB=/path/to/other/libdcfp_hip.so python tools/conv_routes.py > a.txt
    python tools/conv_routes.py > b.txt && cmp a.txt b.txt
The environment knobs latch on first use: one process per setting.
Descriptors: tests/_wp_cases.CASES and sweep(4000, seed), tests/_narrow_cases.NARROW, and every narrow conv of the slim
fixtures at both geometries; each dense and with the row pitch ops.conv_pitch gives it."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

PASSES = ("fwd", "dgrad", "wgrad")
WP_FIELDS = ("n_blocks", "T", "Ck", "CkP", "M", "Mpad", "sAm", "sAc", "perm8")


def cases(seed):
    import _narrow_cases as nc
    import _wp_cases as wc
    out = [c for c, _, _ in wc.CASES] + wc.sweep(4000, seed) + [c for c, _, _, _ in nc.NARROW]
    for npz in nc.fixtures():
        for geometry in nc.GEOMETRIES:
            out += list(nc.slim_convs(npz, geometry))
    return list(dict.fromkeys(out))


def report(case, pitch, out):
    from dcfp_amd import _lib, ops
    L = _lib.lib()
    N, Cin, H, W, Cout, k, s, p, dil = case
    d = ops._desc((N, Cin, H, W), (Cout, Cin, k, k), s, p, dil, pitch, pitch)
    r = C.byref(d)
    tag = " ".join(map(str, case)) + f" pitch={pitch}"
    out.write(f"{tag} | pitch_supported={L.dcfp_conv2d_pitch_supported(r)} "
              f"fwd_stat_slots={L.dcfp_conv2d_fwd_stat_slots(r, None, 0)} "
              f"fanin={L.dcfp_conv2d_dgrad_fanin_supported(r)} fanin_red_slots={L.dcfp_conv2d_dgrad_fanin_red_slots(r)} "
              f"xform_bytes={L.dcfp_conv2d_xform_bytes(r)}\n")
    for which, name in enumerate(PASSES):
        line = (f"{tag} {name} | {ops.conv_kernel_name(d, which)} | exec={ops.conv_executed_fraction(d, which)!r} "
                f"ws={L.dcfp_conv2d_workspace_bytes(r, which)} scratch={L.dcfp_conv2d_workspace_is_scratch(r, which)}")
        if which < 2:
            e = _lib.WpEntry()
            rc = L.dcfp_conv2d_wp_layout(r, which, C.byref(e))
            line += f" | wp rc={rc}" + ("".join(f" {f}={getattr(e, f)}" for f in WP_FIELDS) if rc == 0 else "")
        out.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=20261018, help="seed of the descriptor sweep")
    args = ap.parse_args()
    from dcfp_amd import ops
    for case in cases(args.seed):
        N, Cin, H, W, Cout, k, s, p, dil = case
        report(case, 0, sys.stdout)
        pitch = ops.conv_pitch((N, Cin, H, W), (Cout, Cin, k, k), s, p, dil)
        if pitch:
            report(case, pitch, sys.stdout)


if __name__ == "__main__":
    main()
