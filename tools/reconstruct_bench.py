"""The decode on the device, measured: lsq_index_reconstruct on device arrays against three yardsticks, none of them the code under test,
ALTERNATED with it in one process -- a device-to-device torch copy (16 bytes per lane) of the same output bytes, the torch expression the resident trainers
use today (`dK[dB + offs].sum(dim=1)`, with its peak memory), and the numpy mirror reference_api.reconstruct with the download of the codes and the upload
of the result that it implies for a resident index.  One JSON line per measurement, written to profiles/reconstruct.jsonl and printed.

    python tools/reconstruct_bench.py [--n 1000000]

Device events around every call, medians of 5 after one warm-up.  kernel_ms is the decode kernel alone (lsq_index_recon_info.decode_ms with option
"profile": events on the stream right around the launch); index_call_ms is an event pair around the Python call, so it carries the binding's overhead,
the profile events and the call's wait.
stored_GBps = n d 4 / kernel_ms, gathered_GBps = n m d 4 / kernel_ms (the codeword bytes the lanes load, wherever they are served from)."""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
lsq = importlib.import_module("local-search-quantization_amd")
import recon_check as RC  # noqa: E402
REPS, H, NLIST = 5, 256, 1024
med = statistics.median


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def alternated(**fns):
    """every function once as a warm-up, then REPS rounds in which each runs once, in turn -> {name: median ms}"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for k, f in fns.items():
            ms[k].append(timed(f)[0])
    return {k: med(v) for k, v in ms.items()}


def shape_point(eng, dev, g, n, d, m, packed, emit, numpy_rows):
    name = "%s-m%d-d%d" % ("packed" if packed else "plain", m, d)
    K = (torch.randn((m * H, d), device=dev, generator=g) / m ** 0.5).contiguous()
    rows = torch.randint(0, 256, (n, m + 1), device=dev, generator=g, dtype=torch.uint8)
    codes = rows[:, :m].contiguous()
    out = torch.empty((n, d), device=dev)
    src, dst = torch.empty_like(out), torch.empty_like(out)
    offs = (torch.arange(m, device=dev, dtype=torch.int64) * H)[None, :]
    torch_sum = lambda: K[codes.to(torch.int64) + offs].sum(dim=1)      # noqa: E731 -- the trainers' expression
    nc, cb = torch.zeros(n, dtype=torch.uint8, device=dev), torch.ones(1, device=dev)
    ix = eng.index_packed_dev(codes, K, nc, cb, m) if packed else eng.index_dev(codes, K, torch.zeros(n, device=dev), m)
    kern = []

    def decode_index():
        ix.reconstruct(out=out)
        kern.append(ix.recon_info()["decode_ms"])

    with ix:
        eng.set_option("profile", 1)
        ms = alternated(index_call=decode_index, copy=lambda: dst.copy_(src), torch_sum=torch_sum)
        eng.set_option("profile", 0)
        k_ms = med(kern[1:])
        # the bits: the kernel against the contract on a prefix, the torch expression against it too (its add order is not pinned: reported, not asserted)
        pre = min(n, 20000)
        want = RC.decode(codes[:pre].cpu().numpy(), K.cpu().numpy(), m)
        assert RC.same_bits(out[:pre].cpu().numpy(), want)
        torch_same = bool(RC.same_bits(torch_sum()[:pre].cpu().numpy(), want))
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        r = torch_sum()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del r
        # the numpy mirror for a resident index: codes down, the host loop, the result up (a prefix where the whole set would take minutes; scaled)
        nn_ = min(n, numpy_rows)
        Cs = [np.ascontiguousarray(K[j * H:(j + 1) * H].cpu().numpy().T) for j in range(m)]
        t0 = time.perf_counter()
        B = codes[:nn_].cpu().numpy().astype(np.int16).T + 1
        CB = lsq.reconstruct(B, Cs)
        up = torch.from_numpy(np.ascontiguousarray(CB.T)).to(dev)
        torch.cuda.synchronize()
        numpy_ms = (time.perf_counter() - t0) * 1e3 * (n / nn_)
        del up
        line = dict(bench="reconstruct", what="shape", format=name, n=n, d=d, m=m, reps=REPS, kernel_ms=round(k_ms, 4),
                    index_call_ms=round(ms["index_call"], 4), copy_ms=round(ms["copy"], 4), torch_sum_ms=round(ms["torch_sum"], 4),
                    torch_sum_peak_bytes=int(peak), torch_sum_same_bits_on_prefix=torch_same, numpy_roundtrip_ms=round(numpy_ms, 1), numpy_rows_measured=nn_,
                    out_bytes=n * d * 4, gathered_bytes=n * m * d * 4, table_bytes=m * H * d * 4, stored_GBps=round(n * d * 4 / k_ms / 1e6, 1),
                    copy_GBps_one_way=round(n * d * 4 / ms["copy"] / 1e6, 1), gathered_GBps=round(n * m * d * 4 / k_ms / 1e6, 1),
                    kernel_over_copy=round(k_ms / ms["copy"], 3), torch_sum_over_kernel=round(ms["torch_sum"] / k_ms, 2), road=ix.recon_info()["road"])
        emit(line)
        return line


def index_points(eng, dev, g, n, d, m, emit):
    """the id form, the coarse add with its map, search_rows next to search"""
    K = (torch.randn((m * H, d), device=dev, generator=g) / m ** 0.5).contiguous()
    codes = torch.randint(0, 256, (n, m), device=dev, generator=g, dtype=torch.uint8)
    cent = torch.randn((NLIST, d), device=dev, generator=g)
    assign = torch.randint(0, NLIST, (n,), device=dev, generator=g, dtype=torch.int32)
    norms = torch.rand(n, device=dev, generator=g)
    eng.set_option("profile", 1)
    with eng.index_dev(codes, K, norms, m) as ix:
        ix.set_lists(cent, assign)
        out = torch.empty((n, d), device=dev)
        for count in (1000, 100000):
            ids = torch.randint(0, n, (count,), device=dev, generator=g, dtype=torch.int32)
            o = out[:count]
            kern, calls = [], []
            for _ in range(REPS + 1):
                calls.append(timed(lambda: ix.reconstruct(ids=ids, out=o))[0])
                kern.append(ix.recon_info()["decode_ms"])
            emit(dict(bench="reconstruct", what="ids", n=n, d=d, m=m, count=count, kernel_ms=round(med(kern[1:]), 4), call_ms=round(med(calls[1:]), 4),
                      stored_GBps=round(count * d * 4 / med(kern[1:]) / 1e6, 1), gathered_GBps=round(count * m * d * 4 / med(kern[1:]) / 1e6, 1)))
        plain, coarse, maps = [], [], []
        for _ in range(REPS + 1):
            ix.reconstruct(out=out)
            plain.append(ix.recon_info()["decode_ms"])
            ix.set_lists(cent, assign)                                       # the layout is rebuilt: the next coarse decode derives the map again
            ix.reconstruct(out=out, add_coarse=True)
            info = ix.recon_info()
            assert info["map_rebuilt"] == 1
            coarse.append(info["decode_ms"])
            maps.append(info["map_ms"])
        emit(dict(bench="reconstruct", what="coarse", n=n, d=d, m=m, nlist=NLIST, plain_kernel_ms=round(med(plain[1:]), 4), coarse_kernel_ms=round(med(coarse[1:]), 4),
                  coarse_extra_ms=round(med(coarse[1:]) - med(plain[1:]), 4), map_rebuild_ms=round(med(maps[1:]), 4)))
        eng.set_option("profile", 0)
        for nq in (100, 10000):
            rows = torch.randint(0, n, (nq,), device=dev, generator=g, dtype=torch.int32)
            q = ix.reconstruct(ids=rows)
            for nprobe in (0, 16):
                if nprobe:
                    ms = alternated(search_rows=lambda: ix.search_rows(rows, 10, nprobe=nprobe), search=lambda: ix.search_ivf(q, 10, nprobe))
                else:
                    ms = alternated(search_rows=lambda: ix.search_rows(rows, 10), search=lambda: ix.search(q, 10))
                emit(dict(bench="reconstruct", what="search_rows", n=n, d=d, m=m, nq=nq, nn=10, nprobe=nprobe, search_rows_ms=round(ms["search_rows"], 4),
                          search_ms=round(ms["search"], 4), decode_share_ms=round(ms["search_rows"] - ms["search"], 4)))


def main(n):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(2400)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    f = open(os.path.join(ROOT, "profiles", "reconstruct.jsonl"), "w")

    def emit(line):
        line["device"] = torch.cuda.get_device_name(0)
        s = json.dumps(line)
        print(s, flush=True)
        f.write(s + "\n")
        f.flush()

    with lsq.Engine(0) as eng:
        for d, m, packed, numpy_rows in ((128, 8, False, n), (128, 16, False, n), (960, 8, False, n // 10), (128, 7, True, n)):
            shape_point(eng, dev, g, n, d, m, packed, emit, numpy_rows)
            torch.cuda.empty_cache()
        index_points(eng, dev, g, n, 128, 8, emit)
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    main(ap.parse_args().n)
