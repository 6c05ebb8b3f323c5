"""Lab: workgroup shapes of the token-block gather (tools/lab/gather_lab.hip) against torch.index_select, 64 rows
of [N, 1024] f32 a call, 100 calls queued back to back, five alternated rounds; microseconds per call as
[median, min, max].  Builds the lab library beside this file on first use (hipcc, gfx950).

    python tools/lab/gather_lab.py [out.json]
"""
import ctypes as C, json, os, statistics, subprocess, sys, time
import torch
here = os.path.dirname(os.path.abspath(__file__))
so = os.path.join(here, "libgather_lab.so")
if not os.path.exists(so):
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-std=c++17",
                    os.path.join(here, "gather_lab.hip"), "-o", so], check=True)
lib = C.CDLL(so)
lib.gb_lab.argtypes = [C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 4
lib.gb_lab.restype = C.c_int
dev = torch.device("cuda", 0)
res = {}
for n_src, N in ((512, 257), (1854, 257), (512, 577)):
    W, b, calls = 1024, 64, 100
    x = torch.randn(n_src, N, W, device=dev)
    g = torch.Generator().manual_seed(3)
    didx = [torch.randperm(n_src, generator=g)[:b].to(dev) for _ in range(calls)]
    out = torch.empty(b, N, W, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    want = torch.index_select(x, 0, didx[0])
    names = {0: "256x8", 1: "256x4", 2: "256x2", 3: "256x1", 4: "256x4 ntload", 5: "256x4 ntload+ntstore", 6: "512x4",
             7: "1024x2", 8: "1024x4", 9: "256x2 ntload", 10: "512x2", 11: "256x16"}
    fns = {"torch.index_select": lambda k: torch.index_select(x, 0, didx[k], out=out)}
    for v, nm in names.items():
        out.zero_()
        rc = lib.gb_lab(v, b, N * W, x.data_ptr(), didx[0].data_ptr(), out.data_ptr(), st)
        assert rc == 0 and torch.equal(out, want), nm
        fns[nm] = (lambda v: lambda k: lib.gb_lab(v, b, N * W, x.data_ptr(), didx[k].data_ptr(), out.data_ptr(), st))(v)
    us = {k: [] for k in fns}
    for _ in range(5):
        for nm, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(calls):
                fn(k)
            torch.cuda.synchronize()
            us[nm].append((time.perf_counter() - t0) / calls * 1e6)
    res[f"src{n_src}x{N}"] = {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in us.items()}
    for k, v in res[f"src{n_src}x{N}"].items():
        print(n_src, N, k, v, flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(res, fh, indent=1)
