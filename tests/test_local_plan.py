"""CPU: the launch plan of the fused local-window kernel (lf_plan, cvpr2020_manet_amd/csrc/local_geom.h) -- padded planes, tile
counts, XCD regions, grid, threads, dynamic LDS bytes, the host tile table, images per pair -- and, for the same shapes, the stored
volumes' bytes, the local workspace, the backward workspace and local_dist_kernel's launch (dist_launch).  The plan is what the
launcher, the pooling pass and manet_local_volume_bytes[_f16] read: a plan that disagrees with the kernel's `vimg` index is an
out-of-bounds write into a caller's volume, a host table that disagrees with the device's moves tile boundaries silently.

The header holds no kernel, so a host-only program that includes it compiles in a second or two and runs without a GPU.

EXPECTED was printed by the commit BEFORE the plan existed, from that commit's own csrc/local_match.hip (included whole in a small
program, with stub definitions of manet_frame_layout and manet_mt_launch_local_min_arg): launch_fused_d's own expressions for the
tiles, regions, grid, LDS and host table, lf_images, manet_local_volume_bytes[_f16], manet_local_workspace_bytes,
manet_local_match_backward_workspace_bytes and dist_launch.  It is not regenerated from the code under test: a change of a figure
here is a change of a launch or of the ABI.

Fields: pad = hp,wp,HPAD,WS,plane; tiles = ntx,nty,rw,rh; gy = grid y of (fused, volume-out with 3 pairs, volume-in); lds / attr =
fused / volume-in fp32 / volume-in fp16 (the launch's bytes / the kernel's attribute); tab = host-table entries (0: the device's
table is read); elems = elements per image fp32/fp16; vol = stored-volume bytes fp32/fp16; dist = grid x x y, LDS on the pooled grid."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "cvpr2020_manet_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# (label, h, w, C, d, n_ids, expected): every window radius on a small odd grid; odd sizes with more ids than one per-pixel pass
# (LF_NIP = 8); the smallest legal frame; the 480p and 720p grids of tests/test_gpu_local.py; a pooled width (1500) whose table does
# not fit LF_TAB_MAX: the n = 0 arm
CASES = [
    ("w12x15 d0", 12, 15, 16, 0, 2,
     "pad=6,7,18,24,432 tiles=1,1,1,1 grid=8 gy=1,3,1 nt=256 lds=77824/16096/15072 attr=77824/37600/36576 tab=4 images=1 elems=768/768 vol=4096/2560 ws=55552 bwd_ws=11008 dist=1x1,51200 tabv=0,12,0,15"),
    ("w12x15 d1", 12, 15, 16, 1, 2,
     "pad=6,7,18,28,504 tiles=1,1,1,1 grid=8 gy=1,3,1 nt=256 lds=81920/19712/15616 attr=81920/38144/34048 tab=4 images=1 elems=2048/1920 vol=9216/4864 ws=66048 bwd_ws=12288 dist=1x1,62976 tabv=0,12,0,15"),
    ("w12x15 d2", 12, 15, 16, 2, 2,
     "pad=6,7,16,28,448 tiles=1,2,1,1 grid=8 gy=1,3,1 nt=256 lds=59392/31744/20480 attr=59392/44032/32768 tab=5 images=2 elems=5888/5760 vol=48128/24064 ws=61696 bwd_ws=15104 dist=1x1,59200 tabv=0,11,12,0,15"),
    ("w12x15 d3", 12, 15, 16, 3, 2,
     "pad=6,7,16,32,512 tiles=1,2,1,1 grid=8 gy=1,3,1 nt=512 lds=61440/28192/17952 attr=61440/37408/27168 tab=5 images=2 elems=5376/5376 vol=44032/22528 ws=73984 bwd_ws=19200 dist=1x2,60800 tabv=0,7,12,0,15"),
    ("w12x15 d4", 12, 15, 16, 4, 2,
     "pad=6,7,17,32,544 tiles=1,3,1,2 grid=16 gy=1,3,1 nt=512 lds=63488/27600/17360 attr=63488/35280/25040 tab=6 images=3 elems=5376/5184 vol=65536/32128 ws=83456 bwd_ws=24576 dist=1x2,62400 tabv=0,5,9,12,0,15"),
    ("w12x15 d5", 12, 15, 16, 5, 2,
     "pad=6,7,21,36,756 tiles=1,2,1,1 grid=8 gy=1,3,1 nt=512 lds=100352/51360/29856 attr=100352/62112/40608 tab=5 images=2 elems=10752/10560 vol=87040/43264 ws=117248 bwd_ws=31232 dist=1x3,64768 tabv=0,9,12,0,15"),
    ("w12x15 d6", 12, 15, 16, 6, 2,
     "pad=6,7,22,36,792 tiles=1,2,1,1 grid=8 gy=1,3,1 nt=512 lds=102400/74400/41632 attr=102400/83616/50848 tab=5 images=2 elems=16640/16640 vol=134144/67584 ws=129792 bwd_ws=39168 dist=1x3,64448 tabv=0,7,12,0,15"),
    ("w12x15 d7", 12, 15, 16, 7, 2,
     "pad=6,7,24,40,960 tiles=1,2,1,1 grid=8 gy=1,3,1 nt=256 lds=129024/85088/47200 attr=129024/94304/56416 tab=5 images=2 elems=19200/19200 vol=154624/77824 ws=160768 bwd_ws=48640 dist=1x3,65280 tabv=0,7,12,0,15"),
    ("w12x15 d8", 12, 15, 16, 8, 2,
     "pad=6,7,25,40,1000 tiles=1,3,1,2 grid=16 gy=1,3,1 nt=256 lds=126976/73328/40560 attr=126976/81008/48240 tab=6 images=3 elems=16384/16320 vol=197632/98944 ws=176640 bwd_ws=59392 dist=1x6,62720 tabv=0,5,9,12,0,15"),
    ("w12x15 d9", 12, 15, 16, 9, 2,
     "pad=6,7,27,44,1188 tiles=1,3,1,2 grid=16 gy=1,3,1 nt=256 lds=129024/82032/45168 attr=129024/89712/52848 tab=6 images=3 elems=18432/18240 vol=222208/110464 ws=212736 bwd_ws=71424 dist=1x6,61600 tabv=0,5,9,12,0,15"),
    ("w12x15 d10", 12, 15, 16, 10, 2,
     "pad=6,7,29,56,1624 tiles=1,3,1,2 grid=16 gy=1,3,1 nt=512 lds=130176/122496/66176 attr=130176/130176/73856 tab=6 images=3 elems=28416/28224 vol=342016/170368 ws=282112 bwd_ws=84992 dist=1x6,61760 tabv=0,5,9,12,0,15"),
    ("w12x15 d11", 12, 15, 16, 11, 2,
     "pad=6,7,34,56,1904 tiles=1,2,1,1 grid=16 gy=1,3,1 nt=512 lds=129024/116832/63584 attr=129024/127584/74336 tab=5 images=4 elems=26880/26880 vol=431104/216064 ws=332800 bwd_ws=99840 dist=1x6,59904 tabv=0,9,12,0,15"),
    ("w12x15 d12", 12, 15, 16, 12, 2,
     "pad=6,7,42,56,2352 tiles=1,1,1,1 grid=40 gy=1,3,1 nt=512 lds=144080/122576/69328 attr=144080/144080/90832 tab=4 images=5 elems=26880/26880 vol=538624/269824 ws=406272 bwd_ws=115968 dist=1x6,65024 tabv=0,12,0,15"),
    ("odd33x47 d4", 33, 47, 100, 4, 9,
     "pad=16,23,27,48,1296 tiles=2,8,1,4 grid=32 gy=1,3,1 nt=512 lds=63488/35280/25040 attr=63488/35280/25040 tab=12 images=16 elems=5376/5184 vol=345088/166912 ws=1156096 bwd_ws=708096 dist=2x6,62400 tabv=0,5,9,13,18,22,26,30,33,0,32,47"),
    ("odd33x47 d11", 33, 47, 100, 11, 9,
     "pad=16,23,44,72,3168 tiles=2,4,1,2 grid=32 gy=1,3,1 nt=512 lds=129024/127584/74336 attr=129024/127584/74336 tab=8 images=16 elems=26880/26880 vol=1721344/861184 ws=3313152 bwd_ws=1367552 dist=2x16,59904 tabv=0,9,18,26,33,0,32,47"),
    ("odd33x47 d12", 33, 47, 100, 12, 9,
     "pad=16,23,52,72,3744 tiles=2,2,1,1 grid=40 gy=1,3,1 nt=512 lds=144080/144080/90832 attr=144080/144080/90832 tab=6 images=20 elems=26880/26880 vol=2151424/1076224 ws=3915264 bwd_ws=1508864 dist=2x16,65024 tabv=0,24,33,0,32,47"),
    ("tiny2x2 d0", 2, 2, 1, 0, 1,
     "pad=1,1,13,20,260 tiles=1,1,1,1 grid=8 gy=1,3,1 nt=256 lds=77824/12512/11488 attr=77824/37600/36576 tab=4 images=1 elems=768/768 vol=4096/2560 ws=2816 bwd_ws=512 dist=1x1,51200 tabv=0,2,0,2"),
    ("g30x40 d11", 30, 40, 100, 11, 3,
     "pad=15,20,43,68,2924 tiles=2,4,1,2 grid=32 gy=1,3,1 nt=512 lds=129024/118624/65376 attr=129024/127584/74336 tab=8 images=16 elems=26880/26880 vol=1721344/861184 ws=2974208 bwd_ws=1114880 dist=2x15,59904 tabv=0,9,17,25,30,0,31,40"),
    ("480p d4", 120, 214, 100, 4, 3,
     "pad=60,107,71,132,9372 tiles=8,30,2,15 grid=240 gy=1,3,1 nt=512 lds=63488/28880/18640 attr=63488/35280/25040 tab=40 images=240 elems=5376/5184 vol=5161984/2489344 ws=9577984 bwd_ws=12352256 dist=7x20,62400 tabv=0,5,9,13,17,21,25,29,33,37,41,45,49,53,57,61,65,69,73,77,81,85,89,93,97,101,105,109,113,117,120,0,31,61,91,121,151,181,211,214"),
    ("480p d12", 120, 214, 100, 12, 3,
     "pad=60,107,96,156,14976 tiles=8,6,2,3 grid=240 gy=1,3,1 nt=512 lds=144080/126160/72912 attr=144080/144080/90832 tab=16 images=240 elems=26880/26880 vol=25805824/12903424 ws=28030976 bwd_ws=26322176 dist=7x60,65024 tabv=0,23,45,67,89,111,120,0,31,61,91,121,151,181,211,214"),
    ("720p d4", 180, 320, 100, 4, 6,
     "pad=90,160,101,184,18584 tiles=11,45,3,23 grid=552 gy=1,3,1 nt=512 lds=63488/32720/22480 attr=63488/35280/25040 tab=58 images=495 elems=5376/5184 vol=10645504/5133184 ws=19533056 bwd_ws=27705600 dist=10x30,62400 tabv=0,5,9,13,17,21,25,29,33,37,41,45,49,53,57,61,65,69,73,77,81,85,89,93,97,101,105,109,113,117,121,125,129,133,137,141,145,149,153,157,161,165,169,173,177,180,0,31,61,91,121,151,181,211,241,271,301,320"),
    ("720p d12", 180, 320, 100, 12, 6,
     "pad=90,160,126,208,26208 tiles=11,9,3,5 grid=600 gy=1,3,1 nt=512 lds=144080/136912/83664 attr=144080/144080/90832 tab=22 images=495 elems=26880/26880 vol=53223424/26612224 ws=56966400 bwd_ws=59040000 dist=10x90,65024 tabv=0,23,45,67,89,111,133,155,177,180,0,31,61,91,121,151,181,211,241,271,301,320"),
    ("720p d12 ids11", 180, 320, 100, 12, 11,
     "pad=90,160,126,208,26208 tiles=11,9,3,5 grid=600 gy=1,3,1 nt=512 lds=144080/144080/90832 attr=144080/144080/90832 tab=22 images=495 elems=26880/26880 vol=53223424/26612224 ws=56966400 bwd_ws=59040000 dist=10x90,65024 tabv=0,23,45,67,89,111,133,155,177,180,0,31,61,91,121,151,181,211,241,271,301,320"),
    ("wide8x3000 d4", 8, 3000, 4, 4, 2,
     "pad=4,1500,15,1524,22860 tiles=100,2,25,1 grid=200 gy=1,3,1 nt=512 lds=63488/27600/17360 attr=63488/35280/25040 tab=0 images=200 elems=5376/5184 vol=4301824/2074624 ws=2675712 bwd_ws=2328064 dist=94x2,62400 tabv="),
]

PROGRAM = """
#include <cstdio>
#include "local_geom.h"
struct Case { const char *label; int h, w, C, d, n_ids; };
static const Case cases[] = {
@CASES@};
int main()
{
    for (const Case &c : cases) {
        const LfPlan F = lf_plan(c.h, c.w, c.d, LF_FUSED, c.n_ids, 4, 1), O = lf_plan(c.h, c.w, c.d, LF_VOL_OUT, 1, 4, 3);
        const LfPlan I = lf_plan(c.h, c.w, c.d, LF_VOL_IN, c.n_ids, 4, 1), I16 = lf_plan(c.h, c.w, c.d, LF_VOL_IN, c.n_ids, 2, 1);
        const PoolPad &G = F.G;
        const DistLaunch DL = dist_launch(G.hp, G.wp, c.d);
        printf("%s: pad=%d,%d,%d,%d,%ld tiles=%d,%d,%d,%d grid=%u gy=%u,%u,%u nt=%d lds=%zu/%zu/%zu attr=%zu/%zu/%zu tab=%d "
               "images=%ld elems=%d/%d vol=%zu/%zu ws=%zu bwd_ws=%zu dist=%ux%u,%zu tabv=",
               c.label, G.hp, G.wp, G.HPAD, G.WS, G.plane, F.ntx, F.nty, F.rw, F.rh, F.grid_x, F.grid_y, O.grid_y, I.grid_y, F.nt, F.lds,
               I.lds, I16.lds, F.lds_attr, I.lds_attr, I16.lds_attr, I.tab.n, F.images, I.img_elems, I16.img_elems,
               lf_volume_bytes(c.h, c.w, c.d, 4), lf_volume_bytes(c.h, c.w, c.d, 2), local_layout(c.h, c.w, c.C, c.d, 1).total,
               local_bwd_ws_bytes(c.h, c.w, c.C, c.d), DL.grid.x, DL.grid.y, DL.lds);
        for (int i = 0; i < I.tab.n; ++i) printf("%s%d", i ? "," : "", I.tab.v[i]);
        // the expressions lf_pool_pad_kernel and the frame prepare evaluate on the device, and the other plans' agreement
        printf(" | ");
        for (int i = 0; i <= I.nty; ++i) printf("%d,", bilin_first(i * (lf_sy(c.d) - 1), G.hp, c.h));
        for (int i = 0; i <= I.ntx; ++i) printf("%s%d", i ? "," : "", bilin_first(i * (LF_SX - 1), G.wp, c.w));
        bool same = F.tab.n == 0 && O.tab.n == 0 && I16.tab.n == I.tab.n && O.grid_x == F.grid_x && I.grid_x == F.grid_x && I16.grid_x == F.grid_x;
        for (int i = 0; i < I.tab.n; ++i) same = same && I16.tab.v[i] == I.tab.v[i];
        printf(" | %s\\n", same ? "modes agree" : "MODES DISAGREE");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("local_plan")
    rows = "".join('    {"%s", %d, %d, %d, %d, %d},\n' % c[:6] for c in CASES)
    src = d / "local_plan.cpp"
    src.write_text(PROGRAM.replace("@CASES@", rows))
    exe = str(d / "local_plan")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, str(src), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout
    return {label: rest.split(" | ") for label, rest in (line.split(": ", 1) for line in out.splitlines())}


def test_every_plan_is_what_the_launchers_computed_before_the_plan_existed(plans):
    assert sorted(plans) == sorted(c[0] for c in CASES)
    bad = [(c[0], plans[c[0]][0], c[6]) for c in CASES if plans[c[0]][0] != c[6]]
    assert not bad, "\n".join("%s:\n  got      %s\n  expected %s" % b for b in bad)
    assert all(p[2] == "modes agree" for p in plans.values()), {k: p[2] for k, p in plans.items()}


def test_host_table_is_the_device_expression(plans):
    """wherever the plan hands the table over as a kernel argument (n > 0) it holds bilin_first(i * TY, hp, h) / bilin_first(i * TX,
    wp, w), the expressions lf_pool_pad_kernel and the frame prepare write the device's table with, evaluated in the same program"""
    with_table = [c[0] for c in CASES if " tab=0 " not in plans[c[0]][0]]
    assert len(with_table) == len(CASES) - 1 and "wide8x3000 d4" not in with_table
    for label in with_table:
        got = plans[label][0].split("tabv=")[1]
        assert got and got == plans[label][1], (label, got, plans[label][1])
