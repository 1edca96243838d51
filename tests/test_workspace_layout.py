"""The workspace layout, pinned byte for byte (no GPU).

SIZES holds what rsort_plan_make / rsort_workspace_size, rsort_partition_workspace_size and rsort_multi_workspace_size
returned BEFORE the host driver's layout became one walk (carve in csrc/rsort_capi.cpp): recorded from the commit
before that change with this file's own `python tests/test_workspace_layout.py`, never from the code under test.
A plan without explicit tiles_per_chunk sizes its chunks from an occupancy query where a device is present, so the
sizes are computed in one child process that sees no device (chunks from the 256-CU, 2-workgroup default).

walk() below restates the layout from DESIGN §3 "Workspace state" on its own: every size must also equal it. For a
partition that is the point -- its plan has no next-digit tables, whatever its bucket bits.

The families `segmented`, `topk` and `topk_rows` (rsort_segmented_workspace_size, rsort_topk_workspace_size with the
route given, rsort_topk_rows_workspace_size) were recorded the same way from the commit before those three layouts
and the sort's became walks over one allocator; seg_walk() and rows_walk() restate the two simple ones. The `multi`
rows of worlds 1, 2, 3 and 16 were recorded from the commit before the multi-GPU driver's layout (multi_bytes in
csrc/rsort_multi.cpp) became a walk over that allocator too."""
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
MULTI_MORE_WORLDS = (1, 2, 3, 16)  # (the gathered sample, and the room to sort it, grow with the world)
# tiles_per_chunk of a sort plan: the library's own choice (0), one tile per chunk (k = 4 at 2^22 + 9 keys: 1025
# chunks, raw next-digit tables; at 2^23 + 9: 2049, tail scans), and 256 chunks where n has the tiles for them
# (k = 8 on line tiles: the digit-group plans)
MODES = ("auto", "one", "c256")
SEG_NSEGS = (0, 1, 1000, 1 << 20, (1 << 31) - 1)
TOPK_NS = (0, 1, 63, 70001, 1 << 20, (1 << 24) + 3, 1 << 30, (1 << 32) - 1)
TOPK_ROUTES = ("select", "sort")  # rs.TOPK_SELECT, rs.TOPK_SORT = 1, 2
ROWS_SHAPES = ((1, 1), (4, 64), (1000, 300), (1 << 20, 64), (4096, 16384), (3, 1 << 30))


def al(x):
    return (x + 255) // 256 * 256


def tiles_per_chunk(rs, n, k, pairs, mode):
    if mode == "auto":
        return 0
    if mode == "one":
        return 1
    tile = rs.plan(n, k, pairs, 1).tile_keys
    return max(1, -(-max(1, -(-n // tile)) // 256))


def topk_ks(n):
    return (0, min(n, 64), n // 3, n)


def rows_ks(cols):
    return (1, cols // 4, cols)


def compute():
    """Every size of the grid, from the library as built (run where no device is visible)."""
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from _rs import rs
    lib = rs._lib()
    out = {"sort": {}, "plans": {}, "partition": {}, "multi": {}, "segmented": {}, "topk": {}, "topk_rows": {}}
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
    for world in (MULTI_WORLD,) + MULTI_MORE_WORLDS:
        for k in (8, 4):
            for pairs in (0, 1):
                key = f"k{k} {'pairs' if pairs else 'keys'}" + (f" world {world}" if world != MULTI_WORLD else "")
                out["multi"][key] = [int(lib.rsort_multi_workspace_size(n, rs.default_capacity(n), k, pairs, world))
                                     for n in MULTI_NS]
    for pairs in (0, 1):
        kind = "pairs" if pairs else "keys"
        for nseg in SEG_NSEGS:
            out["segmented"][f"nseg{nseg} {kind}"] = [rs.segmented_workspace_size(n, nseg, bool(pairs)) for n in NS]
        # (the finishing sort's plan sizes its chunks like any sort's: from the occupancy where a device is present)
        for route, name in enumerate(TOPK_ROUTES, start=rs.TOPK_SELECT):
            out["topk"][f"{name} {kind}"] = [[rs.topk_workspace_size(n, k, bool(pairs), route) for k in topk_ks(n)]
                                             for n in TOPK_NS]
        out["topk_rows"][kind] = [[rs.topk_rows_workspace_size(rows, cols, k, bool(pairs)) for k in rows_ks(cols)]
                                  for rows, cols in ROWS_SHAPES]
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
        "k8 keys world 1": [81060608, 81062144, 81992704, 82587904, 119236864, 156872960, 194784000, 119235328, 685501184, 9745241856],
        "k8 pairs world 1": [81322752, 81324800, 83155200, 84325120, 157137664, 232742656, 308292352, 157135616, 1289765632, 19409182464],
        "k4 keys world 1": [17047552, 17047808, 17447680, 17703168, 46753024, 84500992, 122259200, 46751744, 612995840, 9672694784],
        "k4 pairs world 1": [17047552, 17048064, 17847808, 18358784, 84708608, 160205824, 235705600, 84707328, 1217173760, 19336567808],
        "k8 keys world 2": [85254912, 85256448, 86187008, 86782208, 123431168, 161067264, 198978304, 123429632, 689695488, 9749436160],
        "k8 pairs world 2": [85517056, 85519104, 87349504, 88519424, 161331968, 236936960, 312486656, 161329920, 1293959936, 19413376768],
        "k4 keys world 2": [25698304, 25698560, 26098432, 26353920, 50947328, 88695296, 126453504, 50946048, 617190144, 9676889088],
        "k4 pairs world 2": [25698304, 25698816, 26498560, 27009536, 88902912, 164400128, 239899904, 88901632, 1221368064, 19340762112],
        "k8 keys world 3": [89449216, 89450752, 90381312, 90976512, 127625472, 165261568, 203172608, 127623936, 693889792, 9753630464],
        "k8 pairs world 3": [89711360, 89713408, 91543808, 92713728, 165526272, 241131264, 316680960, 165524224, 1298154240, 19417571072],
        "k4 keys world 3": [33955840, 33956096, 34355968, 34611456, 55141632, 92889600, 130647808, 55140352, 621384448, 9681083392],
        "k4 pairs world 3": [33955840, 33956352, 34756096, 35267072, 93097216, 168594432, 244094208, 93095936, 1225562368, 19344956416],
        "k8 keys world 16": [143975168, 143976704, 144907264, 145502464, 182151424, 219787520, 257698560, 182149888, 748415744, 9808156416],
        "k8 pairs world 16": [144237312, 144239360, 146069760, 147239680, 220052224, 295657216, 371206912, 220050176, 1352680192, 19472097024],
        "k4 keys world 16": [143138816, 143139072, 143538944, 143794432, 159916288, 176693504, 193470464, 159916032, 675910400, 9735609344],
        "k4 pairs world 16": [143138816, 143139328, 143939072, 144450048, 176693760, 223120384, 298620160, 176693248, 1280088320, 19399482368],
    },
    "segmented": {
        "nseg0 keys": [256, 512, 400384, 655872, 16777728, 33554944, 50331904, 16777472, 268435712, 4294967552, 17179869440],
        "nseg1 keys": [1280, 1536, 401408, 656896, 16778752, 33555968, 50332928, 16778496, 268436736, 4294968576, 17179870464],
        "nseg1000 keys": [16640, 16896, 416768, 672256, 16794112, 33571328, 50348288, 16793856, 268452096, 4294983936, 17179885824],
        "nseg1048576 keys": [16777472, 16777728, 17177600, 17433088, 33554944, 50332160, 67109120, 33554688, 285212928, 4311744768, 17196646656],
        "nseg2147483647 keys": [34359738624, 34359738880, 34360138752, 34360394240, 34376516096, 34393293312, 34410070272, 34376515840, 34628174080, 38654705920, 51539607808],
        "nseg0 pairs": [256, 768, 800512, 1311488, 33555200, 67109632, 100663552, 33554688, 536871168, 8589934848, 34359738624],
        "nseg1 pairs": [1280, 1792, 801536, 1312512, 33556224, 67110656, 100664576, 33555712, 536872192, 8589935872, 34359739648],
        "nseg1000 pairs": [16640, 17152, 816896, 1327872, 33571584, 67126016, 100679936, 33571072, 536887552, 8589951232, 34359755008],
        "nseg1048576 pairs": [16777472, 16777984, 17577728, 18088704, 50332416, 83886848, 117440768, 50331904, 553648384, 8606712064, 34376515840],
        "nseg2147483647 pairs": [34359738624, 34359739136, 34360538880, 34361049856, 34393293568, 34426848000, 34460401920, 34393293056, 34896609536, 42949673216, 68719476992],
    },
    "topk": {
        "select keys": [[2150656, 2150656, 2150656, 2150656], [2150912, 2151424, 2150912, 2151424], [2150912, 2151424, 2151424, 2151424], [2430720, 2431232, 2622720, 3008256], [6344960, 6345472, 9228544, 14994688], [69259776, 69260288, 114465280, 203827200], [4297117952, 4297118464, 7160950016, 12887575808], [17182019840, 17182020352, 28635789568, 51542281472]],
        "sort keys": [[3328, 3328, 3328, 3328], [3840, 3840, 3840, 3840], [3840, 3840, 3840, 3840], [580864, 580864, 580864, 580864], [8653056, 8653056, 8653056, 8653056], [134570752, 134570752, 134570752, 134570752], [8590461184, 8590461184, 8590461184, 8590461184], [34360264960, 34360264960, 34360264960, 34360264960]],
        "select pairs": [[2150656, 2150656, 2150656, 2150656], [2151168, 2152192, 2151168, 2152192], [2151168, 2152192, 2152192, 2152192], [2710784, 2711808, 3089664, 3848448], [10539264, 10540288, 16219392, 27577600], [136368896, 136369920, 226197248, 405224192], [8592085248, 8592086272, 14319229184, 25772477696], [34361889024, 34361890048, 57268905216, 103081889024]],
        "sort pairs": [[3328, 3328, 3328, 3328], [4352, 4352, 4352, 4352], [4352, 4352, 4352, 4352], [1140992, 1140992, 1140992, 1140992], [17041664, 17041664, 17041664, 17041664], [268858624, 268858624, 268858624, 268858624], [17180395776, 17180395776, 17180395776, 17180395776], [68720003328, 68720003328, 68720003328, 68720003328]],
    },
    "topk_rows": {
        "keys": [[2304, 2048, 2304], [2304, 2304, 3072], [25344, 321280, 1221376], [25166848, 88081408, 289408000], [99328, 67191808, 268518400], [2304, 3221227520, 12884903936]],
        "pairs": [[2560, 2048, 2560], [2560, 2560, 4096], [29440, 621312, 2421504], [29361152, 155190272, 557843456], [115712, 134300672, 536953856], [2560, 6442452992, 25769805824]],
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


SEG_KINDS = 4  # one list per kernel kind of the segmented sort, room for every segment in each


def seg_walk(n, nseg, pairs):
    b = al(4 * n) * (2 if pairs else 1)        # the multi-tile path's ping-pong keys (and values)
    b += SEG_KINDS * al(4 * nseg)              # the kinds' segment lists
    return b + 256                             # counters and check word


def rows_walk(rows, k, pairs):
    b = 256                                    # state words
    b += al(4 * (rows + 1))                    # the finishing sort's offsets
    b += seg_walk(rows * k, rows, pairs)       # the segmented sort of rows segments of k entries
    return b + 256                             # slack: the regions start at the caller's pointer rounded up to 256


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


# What the multi-GPU sort's control area has gained since SIZES was recorded: one 256-B region for the check slots
# of its local sorts (kCheckSlots words, csrc/rsort_multi.cpp), whatever n, capacity, k, pairs and world.
MULTI_CHECK_SLOT_BYTES = 256


def test_multi_workspace_sizes_unchanged():
    """Byte for byte the recorded sizes plus the check slots' one region: rsort_multi_workspace_size covers them."""
    got = computed()["multi"]
    assert set(got) == set(SIZES["multi"])
    for key, want in SIZES["multi"].items():
        assert got[key] == [w + MULTI_CHECK_SLOT_BYTES for w in want], key


def test_segmented_workspace_sizes_unchanged_and_the_walk():
    got = computed()["segmented"]
    assert set(got) == set(SIZES["segmented"])
    for key, want in SIZES["segmented"].items():
        assert got[key] == want, key
        nseg, pairs = int(key.split()[0][4:]), key.endswith("pairs")
        for n, size in zip(NS, got[key]):
            assert size == seg_walk(n, nseg, pairs), (key, n)


def test_topk_workspace_sizes_unchanged():
    got = computed()["topk"]
    assert set(got) == set(SIZES["topk"])
    for key, want in SIZES["topk"].items():
        assert got[key] == want, key
        assert all(size > 0 for row in got[key] for size in row), key  # (0 is the entry's "bad arguments")


def test_topk_rows_workspace_sizes_unchanged_and_the_walk():
    got = computed()["topk_rows"]
    assert set(got) == set(SIZES["topk_rows"])
    for key, want in SIZES["topk_rows"].items():
        assert got[key] == want, key
        for (rows, cols), row in zip(ROWS_SHAPES, got[key]):
            for k, size in zip(rows_ks(cols), row):
                assert size == rows_walk(rows, k, key == "pairs"), (key, rows, cols, k)


if __name__ == "__main__":
    res = compute()
    if "--json" in sys.argv:
        print(json.dumps(res))
    else:  # the literal above
        print("SIZES = {")
        for fam in ("sort", "partition", "multi", "segmented", "topk", "topk_rows"):
            print(f'    "{fam}": {{')
            for key, row in res[fam].items():
                print(f'        "{key}": {row},')
            print("    },")
        print("}")
