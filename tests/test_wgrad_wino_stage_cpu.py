"""CPU: the stage map of the Winograd weight gradient's cotangent (wgrad_wino_kernel<true, true>), modelled in Python.

The block fetches the cotangent g once per stage of two tile groups: wave a, lane (pixel, channel quad) loads 16 bytes
of unit (group a >> 1, half a & 1, pixel row r) and stores them to LDS; lane (n, h) of every wave reads its 16 values
back.  The per-wave loop (load_group, ROWQ branch) has each lane (n, h) load the same 16 values as dwords.  The model
below writes both address computations down independently, as the kernel has them, and checks for every shape of
tests/wgrad_stage_cases.py, every share of the tiles, every n tile and every stage:

  * every slot of the buffer is written exactly once per stage, 16-byte aligned, and no two lanes of one ds_write_b128
    overlap; the 8-lane groups of the store and the half-waves of the dword reads meet every bank at most once;
  * what a reader (group, n, h, j, r, q) finds in its slot is the float the per-wave loop loads for it: the same offset
    into g, or zero for both (a tile past T);
  * every fetch lies inside the probe's cotangent;
  * the stages of a share are its groups two by two, each once, and the re-requested last stage is never consumed.
"""
import pytest

from wgrad_stage_cases import CASES

MI355X_CUS = 256
OOB = None                   # a load the buffer descriptor answers with zeros


def geometry(spec, cus=MI355X_CUS):
    """run_wgrad_wino / wgrad_wino_splits of csrc/lip_mfma.hip"""
    sg = spec.segs[0]
    H, W, C, N, P = spec.OH, spec.OW, sg.C, spec.N, spec.P
    R = spec.n_img * H * W
    T, TH, TW = R // 4, H // 2, W // 2
    groups = (T + 7) // 8
    blocks, want = (C // 32) * (N // 32) * P, 4 * cus
    S = 1 if blocks >= want else (want + blocks - 1) // blocks
    S = max(1, min(S, groups // 16, 64))
    gps = (groups + S - 1) // S
    gps += gps & 1
    return dict(H=H, W=W, C=C, N=N, T=T, TW=TW, tpi=TH * TW, S=S, gps=gps, g_bytes=R * N * 4)


def tile_base(g, t):
    """float offset of pixel (2 ty, 2 tx), channel 0 of tile t"""
    img, rem = divmod(t, g["tpi"])
    ty, tx = divmod(rem, g["TW"])
    return ((img * g["H"] + 2 * ty) * g["W"] + 2 * tx) * g["N"]


def per_wave_offset(g, m, nt, l31, h, j, r, q):
    """load_group, ROWQ branch: the byte offset lane (l31, h) loads for gr[j][2 r + q] of group m"""
    t = 8 * m + 4 * h
    if t >= g["T"]:
        return OOB
    return (tile_base(g, t) + nt * 32 + l31) * 4 + (2 * j + q) * g["N"] * 4 + r * g["W"] * g["N"] * 4


def stage_store(g, m, nt, a, lane, r):
    """stage_load + stage_write of the stage of groups m, m + 1: (byte offset of the 16 bytes or OOB, first float slot)"""
    px, cq = lane >> 3, lane & 7
    sg_, sh = a >> 1, a & 1
    t = 8 * (m + sg_) + 4 * sh
    slot = (4 * sg_ + 2 * sh) * 256 + px * 32 + cq * 4 + r * 256
    if t >= g["T"]:
        return OOB, slot
    return ((tile_base(g, t) + px * g["N"]) + nt * 32 + cq * 4) * 4 + r * g["W"] * g["N"] * 4, slot


def reader_slot(grp, l31, h, j, r, q):
    """stage_read"""
    return grp * 1024 + h * 512 + l31 + r * 256 + (2 * j + q) * 32


def stages_of(g, z):
    """the first groups of the stages the loop of share z CONSUMES, and every stage it requests"""
    m0, m1 = z * g["gps"], (z + 1) * g["gps"]
    consumed = list(range(m0, m1, 2))
    requested = [m0, m0 + 2 if m0 + 2 < m1 else m1 - 2] + [m + 4 if m + 4 < m1 else m1 - 2 for m in consumed]
    return consumed, requested


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_stage_map(case):
    g = geometry(case.spec)
    assert g["TW"] % 4 == 0 and g["gps"] % 2 == 0 and g["gps"] >= 2
    zero_units = 0
    for z in range(g["S"]):
        consumed, requested = stages_of(g, z)
        # the loop requests stage 0, stage 1, then at iteration i stage i + 2: every consumed stage in order, then repeats
        assert requested[:len(consumed)] == consumed
        assert all(m == consumed[-1] for m in requested[len(consumed):]) and len(requested) == len(consumed) + 2
        for nt in range(g["N"] // 32):
            for m in consumed:
                image = {}                                        # float slot -> byte offset of that float (or OOB)
                for a in range(4):
                    for r in range(2):
                        slots = []
                        for lane in range(64):
                            off, slot = stage_store(g, m, nt, a, lane, r)
                            assert slot % 4 == 0 and 0 <= slot and slot + 4 <= 2048
                            if off is OOB:
                                zero_units += lane == 0
                            else:
                                assert off % 16 == 0 and 0 <= off and off + 16 <= g["g_bytes"], (m, a, lane, r, off)
                            for e in range(4):
                                assert slot + e not in image, f"slot {slot + e} written twice in the stage of group {m}"
                                image[slot + e] = OOB if off is OOB else off + 4 * e
                            slots.append(slot)
                        assert len(set(slots)) == 64                 # no two lanes of one ds_write_b128 collide
                        for grp8 in range(8):                        # ds_write_b128: 8 groups of 8 consecutive lanes
                            banks = [(s + e) % 32 for s in slots[8 * grp8: 8 * grp8 + 8] for e in range(4)]
                            assert len(set(banks)) == 32
                assert sorted(image) == list(range(2048))         # every slot exactly once
                for grp in range(2):
                    for j in range(4):
                        for r in range(2):
                            for q in range(2):
                                for h in range(2):
                                    row = [reader_slot(grp, l31, h, j, r, q) for l31 in range(32)]
                                    assert len({s % 32 for s in row}) == 32         # dword reads: banks per half-wave
                                    for l31, s in enumerate(row):
                                        want = per_wave_offset(g, m + grp, nt, l31, h, j, r, q)
                                        assert image[s] == want, (m, grp, l31, h, j, r, q, image[s], want)
    # the shapes were chosen for it: tiles past T exist wherever the groups do not fill the shares
    assert (zero_units > 0) == (8 * g["gps"] * g["S"] > g["T"])


def test_the_shapes_reach_what_they_are_there_for():
    by = {c.name: geometry(c.spec) for c in CASES}
    g = by["stage_10x8_T60"]
    assert g["T"] == 60 and g["gps"] == 8 and g["TW"] == 4 and g["tpi"] == 20     # half a group past T; group 2 in two images
    g = by["stage_12x8_T72"]
    assert g["T"] == 72 and g["gps"] == 10 and (g["T"] + 7) // 8 == 9             # group 9 exists only as padding
    g = by["stage_8x16_N64"]
    assert g["N"] // 32 == 2 and g["C"] // 32 == 2 and g["N"] * 4 != 128
    g = by["stage_8x8"]
    assert g["gps"] == 2 and g["S"] == 1                                          # one stage
    g = by["stage_32x32_split"]
    assert g["S"] == 8 and g["gps"] == 16


def test_the_model_notices_a_wrong_map():
    """the same checks fail on a map with the two pixel rows exchanged in the store"""
    g = geometry(CASES[0].spec)
    off, slot = stage_store(g, 0, 0, 0, 9, 0)
    off1, slot1 = stage_store(g, 0, 0, 0, 9, 1)
    assert slot1 == slot + 256 and off1 == off + g["W"] * g["N"] * 4
    # reader (group 0, n = 4, h = 0, tile j = 0, q = 1) of row 0 reads lane 9's second float of row 0, not of row 1
    s = reader_slot(0, 4, 0, 0, 0, 1)
    assert s == slot and per_wave_offset(g, 0, 0, 4, 0, 0, 0, 1) == off
    assert per_wave_offset(g, 0, 0, 4, 0, 0, 1, 1) == off1 != off
