"""The retrieval launcher's policy on a CPU: tests/c_abi/grouped_policy_table.cpp is compiled with the host compiler against
foodrec_amd/csrc/m2d_grouped_policy.h (plain C++17, no HIP) and prints the policy's output record for the cases below.

Every expected value is what the launcher's own comments state for a 256-CU part ("64 blocks: 16 ranges", "262 144 users: 2
ranges", "more than 24 576 tiles at E = 64", ...) or what its rules give by hand; none was read off the function's output.
Defaults of a case: E = 64, split bf16, k = 10, 3 125 tiles (100 k dishes), 256 CUs, the engine's option defaults."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (input "key=value ...", expected fields)
CASES = {
    # ---- dish ranges of a pruned launch, E = 64 (the ladder's comment) --------------------------------------------------
    # blocks of 256 users: below 16 384 users, or a catalogue of more than 8 192 tiles, or "topk_block" = 256
    "blocks16": ("nU=4096", dict(ublocks=16, nsplit=32, half=0, WV=8)),
    "blocks32": ("nU=8192", dict(ublocks=32, nsplit=32, half=0)),
    "blocks64_long": ("nU=16384 tiles=10000", dict(ublocks=64, nsplit=16, half=0)),
    "blocks128_long": ("nU=32768 tiles=10000", dict(ublocks=128, nsplit=12, half=0)),
    "blocks256_long": ("nU=65536 tiles=10000", dict(ublocks=256, nsplit=8, half=0)),
    "blocks64_forced": ("nU=16384 topk_block=256", dict(ublocks=64, nsplit=16, half=0)),
    "blocks128_forced": ("nU=32768 topk_block=256", dict(ublocks=128, nsplit=12, half=0)),
    "blocks256_forced": ("nU=65536 topk_block=256", dict(ublocks=256, nsplit=8, half=0)),
    "blocks8": ("nU=2048", dict(ublocks=8, nsplit=64)),
    "user1": ("nU=1", dict(ublocks=1, nsplit=512)),
    "users32": ("nU=32", dict(ublocks=1, nsplit=512)),
    "users64": ("nU=64", dict(ublocks=1, nsplit=512)),
    "users65": ("nU=65", dict(ublocks=1, nsplit=256)),
    "users256": ("nU=256", dict(ublocks=1, nsplit=256)),
    "users1024": ("nU=1024", dict(ublocks=4, nsplit=128)),
    "blocks2": ("nU=512", dict(ublocks=2, nsplit=256)),
    "blocks3": ("nU=768", dict(ublocks=3, nsplit=128)),            # 170 -> whole groups of 64
    "blocks5": ("nU=1280", dict(ublocks=5, nsplit=64)),            # 102 -> 64
    "blocks6": ("nU=1536", dict(ublocks=6, nsplit=64)),            # 85 -> 64
    "blocks7": ("nU=1792", dict(ublocks=7, nsplit=64)),            # 73 -> 64
    "blocks24": ("nU=6144", dict(ublocks=24, nsplit=32)),
    "blocks23": ("nU=5888", dict(ublocks=23, nsplit=22)),          # 512 / 23
    "blocks48": ("nU=12288", dict(ublocks=48, nsplit=16)),
    # blocks of 128 users (the launcher's choice from 16 384 users on, up to 8 192 tiles)
    "half16384": ("nU=16384", dict(half=1, WV=4, TPS=4, lds=65536, ublocks=128, nsplit=12)),
    "half131072": ("nU=131072", dict(half=1, ublocks=1024, nsplit=4)),
    "half262144": ("nU=262144", dict(half=1, ublocks=2048, nsplit=2)),
    "half524288": ("nU=524288", dict(half=1, ublocks=4096, nsplit=1, share_thresholds=0)),
    "half98304": ("nU=98304", dict(half=1, ublocks=768, nsplit=4)),
    "half98176": ("nU=98176", dict(half=1, ublocks=767, nsplit=8)),
    # long catalogues: 16 ranges for 192 .. 767 blocks from 16 384 tiles on (E = 64, split bf16); 8 stays beyond
    "long65536": ("nU=65536 tiles=31250", dict(half=0, ublocks=256, nsplit=16)),
    "long65536_16383": ("nU=65536 tiles=16383", dict(ublocks=256, nsplit=8)),
    "long262144": ("nU=262144 tiles=31250", dict(half=0, ublocks=1024, nsplit=8)),
    "long65536_e128": ("nU=65536 tiles=31250 E=128", dict(ublocks=256, nsplit=8)),
    # ---- the clamps on a short catalogue ------------------------------------------------------------------------------
    "stages4": ("nU=4096 tiles=128", dict(nsplit=4)),              # at least four stages (32 tiles) per range
    "stages2": ("nU=4096 tiles=64", dict(nsplit=2)),
    "stages1": ("nU=4096 tiles=40", dict(nsplit=1)),
    "stages_half": ("nU=16384 tiles=128", dict(half=1, nsplit=8)),  # stages of 4 tiles: 16 tiles per range
    "tiles4": ("nU=1 tiles=128", dict(nsplit=32)),                 # at least four tiles per range
    "tiles4_round": ("nU=1 tiles=1000", dict(nsplit=192)),         # 250 -> whole groups of 64
    "tiles4_two": ("nU=1 tiles=8", dict(nsplit=2)),
    "tiles4_one": ("nU=1 tiles=6", dict(nsplit=1)),
    "users300": ("nU=300 tiles=128", dict(ublocks=2, nsplit=32, sorted=1, deal_items=0)),
    # ---- blocks of 128 users: on / off ----------------------------------------------------------------------------------
    "half_8192": ("nU=16384 tiles=8192", dict(half=1, WV=4, TPS=4, lds=65536)),
    "half_8193": ("nU=16384 tiles=8193", dict(half=0, WV=8, TPS=8, lds=131072, ublocks=64)),
    "half_16383": ("nU=16383", dict(half=0, ublocks=64)),
    "half_hook": ("nU=16384 variant=104", dict(half=0, nsplit=4, ublocks=64)),
    "half_apx": ("nU=16384 topk_form=3", dict(apx=1, half=0)),
    "half_unpruned": ("nU=16384 topk_prune=0", dict(half=0)),
    "half_e128": ("nU=16384 E=128", dict(half=0, TPS=4, lds=131072)),
    "half_f32": ("nU=16384 BF16X3=0", dict(half=0)),
    "half_first_form": ("nU=16384 topk_form=1", dict(half=0)),
    "half_compiled_out": ("nU=16384 half_blocks=0", dict(half=0)),
    "block128": ("nU=300 topk_block=128", dict(half=1, WV=4, ublocks=3)),
    "block128_apx": ("nU=300 topk_block=128 topk_form=3", dict(half=0, apx=1, ublocks=2)),
    "block256": ("nU=16384 topk_block=256", dict(half=0, WV=8)),
    # ---- the hi x hi first form -------------------------------------------------------------------------------------------
    "apx64_at": ("nU=65536 tiles=24576", dict(apx=0)),
    "apx64_above": ("nU=65536 tiles=24577", dict(apx=1)),
    "apx128_at": ("nU=65536 tiles=10240 E=128", dict(apx=0)),
    "apx128_above": ("nU=65536 tiles=10241 E=128", dict(apx=1)),
    "apx_hv_at": ("nU=65536 tiles=256 E=32 HV=1", dict(apx=0)),
    "apx_hv_above": ("nU=65536 tiles=257 E=32 HV=1", dict(apx=1)),
    "apx_hv64_above": ("nU=65536 tiles=257 E=64 HV=1", dict(apx=1)),
    "apx_form3": ("nU=300 tiles=128 topk_form=3", dict(apx=1)),
    "apx_form4": ("nU=65536 tiles=31250 topk_form=4", dict(apx=0)),
    "apx_f32": ("nU=65536 tiles=31250 BF16X3=0", dict(apx=0)),
    "apx_first_form": ("nU=65536 tiles=31250 topk_form=1", dict(apx=0)),
    # ---- the first form takes no plan; its split count is the unpruned launch's (1 user: 192) ---------------------------------
    "form1": ("nU=300 topk_form=1", dict(pipe=0, planned=0, ext=0, sorted=0, share_thresholds=0, deal_items=0)),
    "form1_user1": ("nU=1 topk_form=1", dict(planned=0, nsplit=192)),
    "unpruned_user1": ("nU=1 topk_prune=0", dict(planned=1, nsplit=192, pmode=1, sorted=0)),
    "form1_f32": ("nU=300 topk_form=1 BF16X3=0", dict(planned=1, ext=1)),
    "form2": ("nU=300 topk_form=2", dict(pipe=1, planned=1, ext=1)),
    # ---- left-out records ------------------------------------------------------------------------------------------------------
    "ext_default": ("nU=300", dict(ext=1, planned=1, pipe=1)),
    "ext_off": ("nU=300 topk_refine=0", dict(ext=0)),
    "ext_e128_k16": ("nU=300 E=128 k=16", dict(ext=0)),
    "ext_e128_k10": ("nU=300 E=128 k=10", dict(ext=1)),
    "ext_e64_k16": ("nU=300 k=16", dict(ext=1)),
    "ext_hv": ("nU=300 E=32 HV=1", dict(ext=0, pipe=1, sorted=0, pmode=1, share_thresholds=0)),
    "ext_hv_form1": ("nU=300 E=32 HV=1 topk_form=1", dict(pipe=1, planned=1)),
    "ext_pad": ("nU=300 E=200 E8=32 BF16X3=0 PAD=1", dict(ext=0, plan_quads=4)),
    "ext_pad_narrow": ("nU=300 E=100 E8=16 BF16X3=0 PAD=1", dict(ext=0, plan_quads=2)),
    "ext_f32_wide": ("nU=300 E=256 BF16X3=0", dict(ext=0, plan_quads=4)),
    "ext_f32_e128": ("nU=300 E=128 BF16X3=0", dict(ext=1, plan_quads=2)),
    "ext_f32_e32": ("nU=300 E=32 BF16X3=0", dict(ext=1, plan_quads=1, TPS=16, lds=131072)),
    "ext_2p30": ("nU=1073741824", dict(ext=0)),
    "ext_below_2p30": ("nU=1073741823", dict(ext=1)),
    # ---- the split-count hook ("variant" >= 100) ---------------------------------------------------------------------------------
    "hook100": ("nU=300 variant=100", dict(nsplit=1)),
    "hook101": ("nU=300 variant=101", dict(nsplit=1)),
    "hook102": ("nU=300 variant=102", dict(nsplit=2)),
    "hook164": ("nU=300 variant=164", dict(nsplit=64)),
    "hook165": ("nU=300 variant=165", dict(nsplit=64)),
    "hook228": ("nU=300 variant=228", dict(nsplit=128)),
    "hook299": ("nU=300 variant=299", dict(nsplit=192)),
    "hook612": ("nU=300 variant=612", dict(nsplit=512)),
    "hook700": ("nU=300 variant=700", dict(nsplit=512)),
    # ---- probe rows ----------------------------------------------------------------------------------------------------------------
    "probe8191": ("nU=300 tiles=8191", dict(nprobe=16)),
    "probe8192": ("nU=300 tiles=8192", dict(nprobe=32)),
    "probe65535": ("nU=300 tiles=65535", dict(nprobe=32)),
    "probe65536": ("nU=300 tiles=65536", dict(nprobe=64)),
    # ---- test hooks and A/B options ------------------------------------------------------------------------------------------------
    "variant0": ("nU=300", dict(cap=1024, prog_limit=1 << 24, all_patterns=0, pmode=0, sorted=1, share_thresholds=1, deal_items=1)),
    "variant13": ("nU=300 variant=13", dict(cap=2, prog_limit=1 << 24, nsplit=256)),
    "variant15": ("nU=300 variant=15", dict(cap=1024, prog_limit=0, nsplit=256)),
    "prune2": ("nU=300 topk_prune=2", dict(pmode=2)),
    "prune4": ("nU=300 topk_prune=4", dict(pmode=4)),
    "prune5": ("nU=300 topk_prune=5", dict(pmode=0, sorted=1, deal_items=0)),
    "prune7": ("nU=300 topk_prune=7", dict(share_thresholds=0, deal_items=1)),
    "prune9": ("nU=300 topk_prune=9", dict(all_patterns=1, pmode=0)),
    "prune0": ("nU=300 topk_prune=0", dict(pmode=1, sorted=0, deal_items=0, share_thresholds=1)),
    "share_e128": ("nU=300 E=128", dict(share_thresholds=0)),
    "sorted_256": ("nU=256", dict(sorted=0, deal_items=0)),
    "sorted_257": ("nU=257", dict(sorted=1, ublocks=2)),
    "sorted_half_128": ("nU=128 topk_block=128", dict(sorted=0, ublocks=1)),
    "sorted_half_129": ("nU=129 topk_block=128", dict(sorted=1, ublocks=2)),
    "items_at_cus": ("nU=2048 tiles=1024", dict(ublocks=8, nsplit=32, deal_items=0)),      # 256 items: not more than the CUs
    "items_above_cus": ("nU=2304 tiles=1024", dict(ublocks=9, nsplit=32, deal_items=1)),
}


def _build(tmp):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tmp, "grouped_policy_table")
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "c_abi", "grouped_policy_table.cpp"),
           "-I" + os.path.join(ROOT, "foodrec_amd", "csrc"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = _build(str(tmp_path_factory.mktemp("grouped_policy")))
    text = "".join("%s %s\n" % (name, args) for name, (args, _) in CASES.items())
    res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    out = {}
    for line in res.stdout.splitlines():
        name, *fields = line.split()
        out[name] = {f.split("=")[0]: int(f.split("=")[1]) for f in fields}
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_policy_case(table, name):
    got = table[name]
    want = CASES[name][1]
    assert {key: got[key] for key in want} == want, (name, CASES[name][0], got)


def test_split_hook_alone(table):
    # (variant, 7 splits chosen, cap): no hook below 100; 100 -> 0 -> 1; 103 -> 3; 199 -> 99 -> the dense launcher's cap of 64;
    # 700 -> 600 -> the grouped launcher's cap of 512
    assert table["hook"] == dict(v0=7, v100=1, v103=3, v199=64, v700=512)


def test_every_field_is_printed(table):
    fields = {"pipe", "apx", "half", "WV", "TPS", "lds", "ublocks", "nsplit", "planned", "ext", "sorted", "pmode", "nprobe", "plan_quads",
              "share_thresholds", "deal_items", "prog_limit", "all_patterns", "cap"}
    assert set(table["variant0"]) == fields
