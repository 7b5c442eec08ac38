"""Per-shape conv kernel timing with ablation variants (GPU box).

usage: python scripts/conv_bench.py [shapes, e.g. 0,4,7,10,42,43] [variants, e.g. 16,17,18,20]   (sk_bench_conv in include/sidekit_amd.h)

Default variants: the statistics form (conv1 of a block) whole, without stores, without the MFMA loop, without staging; for the
small-grid tilings 42 / 43, which are conv2 only, the residual form likewise (16, 17, 18, 20)."""
import ctypes, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sidekit_amd import _lib
if os.environ.get('SK_LIB'):  # A/B against another build of the library
    _lib.LIB_PATH = os.path.abspath(os.environ['SK_LIB'])
lib = _lib.lib()
torch.cuda.init(); torch.zeros(1).cuda()
names = {i: _lib.PROF_NAMES[i] for i in (0, 2, 4, 5, 7, 8, 10)}
names.update({42: 'conv_L3T (small grid)', 43: 'conv_L4T (small grid)'})
Ts = {0: 401, 2: 401, 4: 201, 5: 201, 7: 101, 8: 101, 10: 51, 42: 101, 43: 51}
shapes = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [0, 4, 7, 10]
STAMPS = os.environ.get("STAMPS", "0") == "1"
variants = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else None
for sh in shapes:
    row = []
    for v in variants or ([16, 17, 18, 20] if sh in (42, 43) else [0, 1, 2, 4]):
        ms = ctypes.c_float(0)
        ph = (ctypes.c_double * 8)()
        try:
            _lib.check(lib.sk_bench_conv(sh, 1, 256, Ts[sh], 20, v, ctypes.byref(ms), ph if STAMPS else None))
        except ValueError:   # e.g. a stride-2 shape has no residual form
            row.append(f"v{v}=n/a")
            continue
        txt = f"v{v}={ms.value*1e3:.0f}us"
        if STAMPS:
            txt += " [cyc: issue %d | land+bar %d | kloop %d | bar+epi %d | bar %d | out %d | WG total %d | clock %.2f GHz]" % (
                ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], ph[7], ph[7] / max(ph[6], 1.0) * 0.1)
        row.append(txt)
    print(names[sh], " ".join(row), flush=True)
