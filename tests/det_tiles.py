"""Python restatement of the output-tile choice of the workgroup-level detector kernels (csrc/engine.cpp det_pick_tile, the instance
tables of csrc/launch_det.inl) and the tiles production runs.  tests/test_op_conformance_det.py forces every one of PRODUCTION_TILES
on a small map, asserts here-equals-engine on the automatic choice (launch log, " tile=THxTW"), and tests/test_gpu_pipeline.py does
the same for the whole 384 x 640 detector."""
import re

# instance -> (S, MAXR, workgroups per CU): PF_DETUNIT_CASE / PF_DETC3_CASE of csrc/launch_det.inl.  det_unit instances are (C, Cin, S) --
# branch channels, block input channels, stride; the kernel's K1 is Cin' rounded up to 32 with Cin' = C (S = 1) or Cin (S = 2).
# det_c3 instances are (CIN, tail) with tail 1 = conv, 2 = detect.
UNIT = {(32, 64, 1): (1, 256, 2), (64, 128, 1): (1, 128, 2), (128, 256, 1): (1, 144, 1),
        (32, 16, 2): (2, 480, 1), (64, 64, 2): (2, 256, 1), (128, 128, 2): (2, 128, 1)}
C3 = {(192, 1): (1, 128, 1), (128, 2): (1, 176, 1)}
INSTANCES = {**{("unit",) + k: v for k, v in UNIT.items()}, **{("c3",) + k: v for k, v in C3.items()}}

# the maps of each instance's launches in the 384 x 640 detector (graph/detector.py): output H x W
PRODUCTION_MAPS = {("unit", 32, 16, 2): [(48, 80)], ("unit", 32, 64, 1): [(48, 80)], ("unit", 64, 64, 2): [(24, 40)],
                   ("unit", 64, 128, 1): [(24, 40)], ("unit", 128, 128, 2): [(12, 20)], ("unit", 128, 256, 1): [(12, 20)],
                   ("c3", 192, 1): [(24, 40)], ("c3", 128, 2): [(48, 80), (24, 40), (12, 20)]}
PRODUCTION_CUS = 256
PRODUCTION_BATCHES = range(1, 33)


def kernel_name(inst):
    """Substring of the launch-log entry of the instance."""
    if inst[0] == "unit":
        _, c, cin, s = inst
        k1 = -(-(c if s == 1 else cin) // 32) * 32
        return "det_unit_kernel<%d, %d, %d, " % (c, k1, s)
    return "det_c3_kernel<%d, %d, " % inst[1:]


def region_rows(th, tw, s):
    return ((th - 1) * s + 3) * ((tw - 1) * s + 3)


def pick_tile(num_cus, out_h, out_w, s, max_rows, batch, wg_per_cu):
    """det_pick_tile, statement by statement (the doubles included: Python floats are the same IEEE doubles)."""
    best, th_best, tw_best = 1e30, 1, 1
    for div in range(1, 17):
        tw = (out_w + div - 1) // div
        if div > 1 and tw == (out_w + div - 2) // (div - 1):
            continue
        rw = (tw - 1) * s + 3
        for th in range(1, out_h + 1):
            rows = ((th - 1) * s + 3) * rw
            if rows > max_rows:
                break
            wgs = batch * ((out_h + th - 1) // th) * ((out_w + tw - 1) // tw)
            rounds = (wgs + num_cus * wg_per_cu - 1) // (num_cus * wg_per_cu)
            cost = float(rounds) * (768.0 + rows) + 0.5 * float(wgs) * rows / num_cus
            if cost < best:
                best, th_best, tw_best = cost, th, tw
    return th_best, tw_best


def pick(inst, num_cus, out_h, out_w, batch):
    s, maxr, per_cu = INSTANCES[inst]
    return pick_tile(num_cus, out_h, out_w, s, maxr, batch, per_cu)


def production_tiles():
    """{instance: sorted [(TH, TW)]} over 256 compute units, the 384 x 640 layer maps and B = 1 .. 32."""
    out = {}
    for inst, maps in PRODUCTION_MAPS.items():
        out[inst] = sorted({pick(inst, PRODUCTION_CUS, h, w, b) for h, w in maps for b in PRODUCTION_BATCHES})
    return out


_NOTE = re.compile(r" tile=(\d+)x(\d+) tpf=(\d+) grid=(\d+)")


def logged_tiles(log, inst=None):
    """[(entry, TH, TW, tiles per frame, grid)] of the det_unit / det_c3 launches of a launch log (of one instance if given)."""
    out = []
    for entry in log:
        if "det_unit_kernel<" not in entry and "det_c3_kernel<" not in entry:
            continue
        if inst is not None and kernel_name(inst) not in entry:
            continue
        m = _NOTE.search(entry)
        assert m, "det launch without its tile note: %r" % entry
        out.append((entry,) + tuple(int(g) for g in m.groups()))
    return out
