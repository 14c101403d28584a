"""Host-side tooling that decides which kernels run: the tuned-table generator's merge rules (CPU only)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entry(shape, cfg, s, us, dus=99.0):
    return {'shape': list(shape) + [0, 0, 0, 0, 0], 'count': 1, 'best_cfg': cfg, 'best_splitk': s, 'best_us': us, 'default_us': dus, 'trials': []}


def test_tuned_table_merge_rules(tmp_path, monkeypatch):
    """Within one sweep generation the fastest measurement of a shape wins; a later generation replaces an entry only when it
    is > 3 % faster; in-eval files (measured against the then-current table in the same run) override unconditionally."""
    a, b, c = (64, 1280, 1280, 0, 0, 0), (128, 640, 640, 0, 0, 0), (256, 320, 320, 0, 0, 0)
    files = {
        'tune2_x.json': {'a': _entry(a, 5, 1, 10.0), 'b': _entry(b, 3, 1, 20.0)},
        'tune2_y.json': {'a': _entry(a, 4, 2, 9.0), 'none': dict(_entry(c, 1, 1, 5.0), best_cfg=None)},
        'tune3_z.json': {'a': _entry(a, 14, 1, 8.9), 'b': _entry(b, 16, 1, 18.0)},       # a: < 3 % better -> stays; b: replaced
        'ineval_q.json': {'a': _entry(a, 19, 4, 50.0)},                                     # slower number, still applied
    }
    paths = []
    for name, d in files.items():
        (tmp_path / name).write_text(json.dumps(d)); paths.append(str(tmp_path / name))
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_tuned_table as g
    out = tmp_path / 'table.inc'
    monkeypatch.setattr(g, 'OUT', str(out))
    monkeypatch.setattr(sys, 'argv', ['gen_tuned_table.py'] + paths)
    g.main()
    rows = [l.split('//')[0].strip() for l in out.read_text().splitlines() if l.startswith('{')]
    assert rows == ['{64, 1280, 1280, 0, 0, 0, 19, 4},', '{128, 640, 640, 0, 0, 0, 16, 1},']


def test_committed_table_matches_its_sources(tmp_path):
    """gemm_tuned.inc is reproducible from the committed sweep files (profiles/tune/*.json)."""
    import glob
    srcs = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'tune', '*.json')))
    assert srcs
    env = dict(os.environ)
    r = subprocess.run([sys.executable, '-c', (
        'import sys, os; sys.path.insert(0, %r); import gen_tuned_table as g; g.OUT = os.devnull if False else %r; '
        'sys.argv = ["x"] + %r; g.main()') % (os.path.join(ROOT, 'tools'), str(tmp_path / 'table.inc'), srcs)],
        capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    strip = lambda t: [l.split('//')[0].strip() for l in t.splitlines() if l.startswith('{')]
    have = strip(open(os.path.join(ROOT, 'makeupdiffuse_amd', 'csrc', 'gemm_tuned.inc')).read())
    want = strip((tmp_path / 'table.inc').read_text())
    assert have == want


def test_tuner_scripts_know_the_librarys_tile_table():
    """Configuration indices are persistent: gemm_tuned.inc and profiles/tune/*.json hold them.  So mkd_gemm_tile_info (host only, no GPU)
    must report exactly these 51 rows - tile M, tile N, LDS-staged conv flag, name, pinned here as literals - and the tuner scripts must
    take the table from the library instead of carrying copies of it."""
    import ctypes as C
    import re
    tile_m = [256, 128, 128, 128, 64, 64, 256, 256, 128, 128, 64, 64, 64, 64, 64, 128, 64, 32, 64, 32,
              32, 32, 64, 64, 64, 64, 32, 32, 128, 64, 64, 128, 64, 64, 128, 128, 64, 64, 128, 64, 128, 256, 256, 128,
              256, 256, 128, 128, 128, 256, 256]
    tile_n = [128, 128, 128, 64, 128, 64, 128, 64, 128, 64, 128, 64, 64, 128, 160, 160, 160, 64, 32, 32,
              32, 32, 32, 32, 64, 64, 64, 64, 64, 128, 64, 64, 128, 32, 128, 64, 128, 64, 64, 128, 128, 64, 128, 128,
              64, 128, 128, 64, 160, 64, 256]
    names = ["256x128", "128x128_s3", "128x128_s2", "128x64", "64x128", "64x64",
             "patch256x128", "patch256x64", "patch128x128", "patch128x64",
             "patch64x128", "patch64x64", "64x64_s6", "64x128_s5", "64x160", "128x160", "64x160_s2", "32x64", "64x32", "32x32",
             "32x32_k2", "32x32_k4", "64x32_k2", "64x32_k4", "64x64_k2", "64x64_k4", "32x64_k2", "32x64_k4", "128x64_k2", "64x128_k2",
             "64x64_s2", "128x64_s2", "64x128_s2", "64x32_s2", "128x128_w8", "128x64_w8", "64x128_w8", "64x64_w8",
             "patch128x64_w8", "patch64x128_w8", "patch128x128_w8", "256x64_w8", "patch256x128_w16", "patch128x128_w16",
             "ra256x64_w8", "ra256x128_w8", "ra128x128", "ra128x64", "ra128x160", "ra256x64", "256x256_w16"]
    patch = {6, 7, 8, 9, 10, 11, 38, 39, 40, 42, 43}
    assert len(tile_m) == len(tile_n) == len(names) == 51
    sys.path.insert(0, ROOT)
    from makeupdiffuse_amd import lib as mlib
    lib = mlib.load()
    assert lib.mkd_gemm_tile_info(-1, None, None, None, None) == 51
    for cfg in range(51):
        m, n, p, nm = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_char_p()
        assert lib.mkd_gemm_tile_info(cfg, C.byref(m), C.byref(n), C.byref(p), C.byref(nm)) == 51
        assert (m.value, n.value, p.value, nm.value.decode()) == (tile_m[cfg], tile_n[cfg], int(cfg in patch), names[cfg]), f'configuration {cfg}'
    for cfg in (-1, 51):          # out of range: the count, outputs untouched
        m = C.c_int(-7)
        assert lib.mkd_gemm_tile_info(cfg, C.byref(m), None, None, None) == 51 and m.value == -7
    assert mlib.tile_table() == [(tile_m[c], tile_n[c], c in patch, names[c]) for c in range(51)]
    for script in ('tune_gemm.py', 'tune_ineval.py', 'tune_wall.py'):
        text = open(os.path.join(ROOT, 'tools', script)).read()
        assert 'tile_table()' in text, f'{script}: does not read the library table'
        assert not re.search(r'\[\s*\d+\s*(,\s*\d+\s*){7,}', text), f'{script}: carries a literal list of numbers'
        assert not re.search(r'\d+\s*<=?\s*cfg|cfg\s*[<>]=?\s*\d+|cfg\s+in\s*[(\[{]\s*\d', text), f'{script}: selects configurations by literal index'
