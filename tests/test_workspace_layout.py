"""The workspace layout, pinned byte for byte (no GPU).

SIZES holds what rsort_plan_make / rsort_workspace_size, rsort_partition_workspace_size and rsort_multi_workspace_size
returned BEFORE the host driver's layout became one walk (carve in csrc/rsort_capi.cpp): recorded from the commit
before that change with this file's own `python tests/test_workspace_layout.py`, never from the code under test.
A plan without explicit tiles_per_chunk sizes its chunks from an occupancy query where a device is present, so the
sizes are computed in one child process that sees no device (chunks from the 256-CU, 2-workgroup default).

walk() below restates the layout from DESIGN §3 "Workspace state" on its own: every size must also equal it. For a
partition that is the point -- its plan has no next-digit tables, whatever its bucket bits."""
import json
import os
import subprocess
import sys
from pathlib import Path

NS = (0, 1, 100003, 4096 * 40 + 3, (1 << 22) + 9, (1 << 23) + 9, 768 * 16384 - 5, 512 * 8192, 1 << 26, 1 << 30,
      (1 << 32) - 1)
KS = (1, 3, 4, 5, 8, 11, 13)
BUCKETS = (2, 8, 17, 32)
MULTI_NS = tuple(n for n in NS if n <= 1 << 30)
MULTI_WORLD = 8
# tiles_per_chunk of a sort plan: the library's own choice (0), one tile per chunk (k = 4 at 2^22 + 9 keys: 1025
# chunks, raw next-digit tables; at 2^23 + 9: 2049, tail scans), and 256 chunks where n has the tiles for them
# (k = 8 on line tiles: the digit-group plans)
MODES = ("auto", "one", "c256")


def al(x):
    return (x + 255) // 256 * 256


def tiles_per_chunk(rs, n, k, pairs, mode):
    if mode == "auto":
        return 0
    if mode == "one":
        return 1
    tile = rs.plan(n, k, pairs, 1).tile_keys
    return max(1, -(-max(1, -(-n // tile)) // 256))


def compute():
    """Every size of the grid, from the library as built (run where no device is visible)."""
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from _rs import rs
    lib = rs._lib()
    out = {"sort": {}, "plans": {}, "partition": {}, "multi": {}}
    for k in KS:
        for pairs in (0, 1):
            for mode in MODES:
                ps = [rs.plan(n, k, bool(pairs), tiles_per_chunk(rs, n, k, bool(pairs), mode)) for n in NS]
                key = f"k{k} {'pairs' if pairs else 'keys'} {mode}"
                out["sort"][key] = [int(p.workspace_bytes) for p in ps]
                out["plans"][key] = [p.as_dict() for p in ps]
                if mode == "auto":
                    assert out["sort"][key] == [rs.workspace_size(n, k, bool(pairs)) for n in NS]
    for nb in BUCKETS:
        for pairs in (0, 1):
            out["partition"][f"b{nb} {'pairs' if pairs else 'keys'}"] = [
                int(lib.rsort_partition_workspace_size(n, nb, pairs)) for n in NS]
    for k in (8, 4):
        for pairs in (0, 1):
            out["multi"][f"k{k} {'pairs' if pairs else 'keys'}"] = [
                int(lib.rsort_multi_workspace_size(n, rs.default_capacity(n), k, pairs, MULTI_WORLD))
                for n in MULTI_NS]
    return out


_computed = None


def computed():
    global _computed
    if _computed is None:
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--json"], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        _computed = json.loads(r.stdout.splitlines()[-1])
    return _computed


SIZES = {
    "sort": {
        "k1 keys auto": [1024, 1280, 401152, 656896, 16780544, 33558272, 50336512, 16782080, 268440320, 4294972160, 17179874048],
        "k1 keys one": [1024, 1280, 401152, 656896, 16782592, 33563904, 50344704, 16782080, 268501760, 4296016640, 17184065024],
        "k1 keys c256": [1024, 1280, 401152, 656896, 16779776, 33557248, 50334464, 16780032, 268438272, 4294970112, 17179872000],
        "k1 pairs auto": [1024, 1536, 801280, 1312512, 33558528, 67113472, 100668160, 33559296, 536875776, 8589939456, 34359743232],
        "k1 pairs one": [1024, 1536, 801280, 1312512, 33564160, 67126784, 100688640, 33563392, 537002752, 8592032768, 34368129536],
        "k1 pairs c256": [1024, 1536, 801280, 1312512, 33557504, 67112192, 100666112, 33557248, 536873728, 8589937408, 34359741184],
        "k3 keys auto": [1536, 1792, 403968, 660992, 16811264, 33595392, 50381568, 16827136, 268485376, 4295017216, 17179919104],
        "k3 keys one": [1536, 1792, 403968, 660992, 16877312, 33752832, 50627328, 16876288, 270009088, 4320135680, 17280541184],
        "k3 keys c256": [1536, 1792, 403968, 660992, 16798208, 33577728, 50356992, 16802560, 268460800, 4294992640, 17179894528],
        "k3 pairs auto": [1024, 1536, 802048, 1313536, 33566720, 67123456, 100680448, 33571584, 536888064, 8589951744, 34359755520],
        "k3 pairs one": [1024, 1536, 802048, 1313536, 33588736, 67175936, 100762368, 33587968, 537395968, 8598325760, 34393301504],
        "k3 pairs c256": [1024, 1536, 802048, 1313536, 33562368, 67117568, 100672256, 33563392, 536879872, 8589943552, 34359747328],
        "k4 keys auto": [1536, 1792, 406272, 664832, 16844288, 33634560, 50430720, 16876288, 268534528, 4295066368, 17179968256],
        "k4 keys one": [1536, 1792, 406272, 664832, 16975616, 33949440, 50922240, 16974592, 271581952, 4307551744, 17230205440],
        "k4 keys c256": [1536, 1792, 406272, 664832, 16818176, 33599232, 50381568, 16827136, 268485376, 4295017216, 17179919104],
        "k4 pairs auto": [1024, 1536, 802816, 1314816, 33577728, 67136512, 100696832, 33587968, 536904448, 8589968128, 34359771904],
        "k4 pairs one": [1024, 1536, 802816, 1314816, 33621504, 67241472, 100860672, 33620736, 537920256, 8606716416, 34426864128],
        "k4 pairs c256": [1024, 1536, 802816, 1314816, 33569024, 67124736, 100680448, 33571584, 536888064, 8589951744, 34359755520],
        "k5 keys auto": [1024, 1280, 404224, 661760, 16822016, 33588480, 50381568, 16843520, 268501760, 4295033600, 17179935488],
        "k5 keys one": [1024, 1280, 404224, 661760, 16909568, 33621248, 50430720, 16909056, 268960512, 4303358464, 17213432320],
        "k5 keys c256": [1024, 1280, 404224, 661760, 16804608, 33577472, 50365184, 16810752, 268468992, 4295000832, 17179902720],
        "k5 pairs auto": [1024, 1536, 804352, 1317376, 33588736, 67153920, 100729600, 33620736, 536937216, 8590000896, 34359804672],
        "k5 pairs one": [1024, 1536, 804352, 1317376, 33621504, 67241472, 100860672, 33620736, 537920256, 8606716416, 34426864128],
        "k5 pairs c256": [1024, 1536, 804352, 1317376, 33577728, 67136512, 100696832, 33587968, 536904448, 8589968128, 34359771904],
        "k8 keys auto": [2816, 3072, 427520, 699392, 17129472, 33819648, 50726656, 17303296, 268961536, 4295493376, 17180395264],
        "k8 keys one": [2816, 3072, 427520, 699392, 17829120, 34081792, 51119872, 17827584, 272632320, 4362094080, 17448371712],
        "k8 keys c256": [2816, 3072, 427520, 699392, 16989184, 33731584, 118786560, 17041152, 336890368, 4363422208, 17248324096],
        "k8 pairs auto": [2816, 3328, 827648, 1355008, 33819904, 67461376, 101189376, 34080512, 537396992, 8590460672, 34360264448],
        "k8 pairs one": [2816, 3328, 827648, 1355008, 34082048, 68161024, 102238208, 34080512, 545263104, 8724186624, 34896741888],
        "k8 pairs c256": [2816, 3328, 827648, 1355008, 33731840, 67321088, 169118208, 102009344, 605325824, 8658389504, 34428193280],
        "k11 keys auto": [17152, 17408, 613888, 1000448, 19588608, 36923136, 54535680, 20981248, 272639488, 4299171328, 17184073216],
        "k11 keys one": [17152, 17408, 613888, 1000448, 25185280, 50353152, 75512320, 25176576, 402694656, 6442983936, 25771909632],
        "k11 keys c256": [17152, 17408, 613888, 1000448, 18466048, 35431680, 52438016, 18883584, 270541824, 4297073664, 17181975552],
        "k11 pairs auto": [17152, 17664, 1014016, 1656064, 36366080, 70477824, 104867328, 37758464, 541074944, 8594138624, 34363942400],
        "k11 pairs one": [17152, 17664, 1014016, 1656064, 41962752, 83907840, 125843968, 41953792, 671130112, 10737951232, 42951778816],
        "k11 pairs c256": [17152, 17664, 1014016, 1656064, 35243520, 68986368, 102769664, 35660800, 538977280, 8592040960, 34361844736],
        "k13 keys auto": [66304, 66560, 1252864, 2032896, 28020224, 47026176, 67146240, 33591808, 285250048, 4311781888, 17196683776],
        "k13 keys one": [66304, 66560, 1252864, 2032896, 50406400, 100746240, 151052800, 50373120, 805470720, 12887032320, 51548029440],
        "k13 keys c256": [66304, 66560, 1252864, 2032896, 23529984, 41061120, 58755584, 25201152, 276859392, 4303391232, 17188293120],
        "k13 pairs auto": [66304, 66816, 1652992, 2688512, 44797696, 80580864, 117477888, 50369024, 553685504, 8606749184, 34376552960],
        "k13 pairs one": [66304, 66816, 1652992, 2688512, 67183872, 134300928, 201384448, 67150336, 1073906176, 17181999616, 68727898624],
        "k13 pairs c256": [66304, 66816, 1652992, 2688512, 40307456, 74615808, 109087232, 41978368, 545294848, 8598358528, 34368162304],
    },
    "partition": {
        "b2 keys": [1024, 1280, 401408, 657152, 16786688, 33566464, 50348800, 16794368, 268452608, 4294984448, 17179886336],
        "b2 pairs": [1024, 1536, 801536, 1312768, 33561344, 67116800, 100672256, 33563392, 536879872, 8589943552, 34359747328],
        "b8 keys": [1024, 1280, 401920, 657920, 16786688, 33566464, 50348800, 16794368, 268452608, 4294984448, 17179886336],
        "b8 pairs": [1024, 1536, 802048, 1313536, 33566720, 67123456, 100680448, 33571584, 536888064, 8589951744, 34359755520],
        "b17 keys": [1024, 1280, 404224, 661760, 16811264, 33599232, 50397952, 16843520, 268501760, 4295033600, 17179935488],
        "b17 pairs": [1024, 1536, 804352, 1317376, 33599488, 67162624, 100729600, 33620736, 536937216, 8590000896, 34359804672],
        "b32 keys": [1024, 1280, 404224, 661760, 16811264, 33599232, 50397952, 16843520, 268501760, 4295033600, 17179935488],
        "b32 pairs": [1024, 1536, 804352, 1317376, 33599488, 67162624, 100729600, 33620736, 536937216, 8590000896, 34359804672],
    },
    "multi": {
        "k8 keys": [110420736, 110422272, 111352832, 111948032, 148596992, 186233088, 224144128, 148595456, 714861312, 9774601984],
        "k8 pairs": [110682880, 110684928, 112515328, 113685248, 186497792, 262102784, 337652480, 186495744, 1319125760, 19438542592],
        "k4 keys": [76029952, 76030208, 76430080, 76685568, 92807424, 113861120, 151619328, 92807168, 642355968, 9702054912],
        "k4 pairs": [76029952, 76030464, 76830208, 77341184, 114068736, 189565952, 265065728, 114067456, 1246533888, 19365927936],
    },
}


# ------------------------------------------------------------------------------ the layout, restated
JOINT_REGIONS = (256 * 256 * 4 + 4,            # joint counts + rows counter
                 2 * (256 + 2 + 4) * 4,        # group bounds of passes 1 and 3: {flag, 257 starts, 4 stats} each
                 (16 + 256 + 256 + 4 * 1024 + 12 * 256) * 4,  # cut plan
                 2 * 256 * 256 * 4,            # piece counts
                 (256 ** 3 + 256 * 256) * 4)   # per-chunk joint-count rows + their one-digit words


def walk(n, pairs, bins, chunks, joint, next_tables):
    entries = bins * chunks
    b = al(4 * n) * (2 if pairs else 1)        # ping-pong keys (and values)
    b += al(4 * entries)                       # chunk x digit table
    b += al(4 * -(-entries // 4096))           # scan block sums
    b += al(4 * (bins + 1))                    # bucket starts
    b += 256                                   # check words
    if joint:
        b += sum(al(x) for x in JOINT_REGIONS)
    if next_tables:
        b += 2 * al(4 * entries)
    return b


def is_joint(p):
    return (p["k_bits"] == 8 and p["num_chunks"] == 256 and p["passes"] >= 2 and p["threads"] == 1024 and
            p["tile_keys"] == (8192 if p["pairs"] else 16384))


def is_next(p):
    return (p["k_bits"] in (3, 4) and not p["pairs"] and p["passes"] >= 2 and
            (p["threads"], p["tile_keys"]) in ((256, 4096), (1024, 16384)))


def partition_shape(n, nb, pairs):
    """(bins, chunks) of a partition plan where no device is visible: 8192-key tiles of 512 threads for keys-only
    inputs of at least two tiles per CU (256 CUs), else 4096-key tiles of 256 threads; at most one wave per digit;
    512 chunks at the most."""
    threads, tile = (512, 8192) if (not pairs and n >= 512 * 8192) else (256, 4096)
    bits = 1
    while (1 << bits) < nb or (threads >> bits) > 64:
        bits += 1
    tiles = max(1, -(-n // tile))
    tpc = -(-tiles // 512)
    return 1 << bits, -(-tiles // tpc)


# ------------------------------------------------------------------------------ tests
def test_sort_workspace_sizes_unchanged():
    got = computed()["sort"]
    assert set(got) == set(SIZES["sort"])
    for key, want in SIZES["sort"].items():
        assert got[key] == want, key


def test_the_grid_reaches_the_routes():
    plans = computed()["plans"]
    assert sum(is_joint(p) for p in plans["k8 keys c256"]) >= 4 and sum(is_joint(p) for p in plans["k8 pairs c256"]) >= 4
    chunks = [p["num_chunks"] for p in plans["k4 keys one"] if is_next(p)]
    assert 1025 in chunks and 2049 in chunks and min(chunks) < 1280 < max(chunks)
    assert any(is_next(p) for p in plans["k3 keys auto"])


def test_sort_workspace_is_the_walk():
    c = computed()
    for key, ps in c["plans"].items():
        for p, size in zip(ps, c["sort"][key]):
            want = walk(p["n"], p["pairs"], p["bins"], p["num_chunks"], is_joint(p), is_next(p))
            assert size == p["workspace_bytes"] == want, (key, p)


def test_partition_workspace_sizes_unchanged_and_the_walk():
    got = computed()["partition"]
    assert set(got) == set(SIZES["partition"])
    small3 = 0
    for key, want in SIZES["partition"].items():
        assert got[key] == want, key
        nb, pairs = int(key.split()[0][1:]), key.endswith("pairs")
        for n, size in zip(NS, got[key]):
            bins, chunks = partition_shape(n, nb, pairs)
            # no next-digit tables: not even for a keys-only partition with 3 or 4 bucket bits on 4096-key tiles
            # (8 buckets of a small input), the shape a next-digit SORT plan has
            small3 += (not pairs and bins in (8, 16) and n < 512 * 8192)
            assert size == walk(n, pairs, bins, chunks, False, False), (key, n)
    assert small3 >= 4


def test_multi_workspace_sizes_unchanged():
    got = computed()["multi"]
    assert set(got) == set(SIZES["multi"])
    for key, want in SIZES["multi"].items():
        assert got[key] == want, key


if __name__ == "__main__":
    res = compute()
    if "--json" in sys.argv:
        print(json.dumps(res))
    else:  # the literal above
        print("SIZES = {")
        for fam in ("sort", "partition", "multi"):
            print(f'    "{fam}": {{')
            for key, row in res[fam].items():
                print(f'        "{key}": {row},')
            print("    },")
        print("}")
