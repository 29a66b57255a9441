"""GPU: the DarkForest extraction beside the AGZ extraction, and forward with and without the placement-ply table, in one process.

(a) eng.extract_df (k_extract_df, fp32 [25][19][19] rows) and eng.extract_agz (k_extract_agz, fp32 [18][19][19] rows) alternating on
    the same 4096 and 16 384 19x19 boards at ply 150 (uniformly random legal moves, one ply per launch on a tracking engine): time
    per call, rows per second, bytes written per second (planes * N*N * 4 per row), that rate over the HBM peak of
    MI355X_MICROARCH.md (8 TB/s) and over the extract_agz rate of the same run;
(b) forward of one ply on a tracking engine (k_forward + k_df_note) and on a plain engine holding the same positions (k_forward),
    alternating.
Times are device events around each call, which ends in a synchronise, after a warm-up; medians of 12.  Writes
profiles/df_bench.json (or the path given as the first argument) and prints the same JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import elf_amd

REPS, WARM = 12, 2
HBM_PEAK = 8.0e12   # bytes per second
N = 19


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, r


def spread(v):
    v = sorted(v)
    return dict(min=v[0], median=v[len(v) // 2], max=v[-1])


def random_moves(eng, gen):
    """one uniformly random legal point per board as a Coord (pass where there is none)"""
    legal = eng.legal_mask()[:, :-1].to(torch.float32)
    none = legal.sum(dim=1) == 0
    legal[none, 0] = 1
    a = torch.multinomial(legal, 1, generator=gen).squeeze(1)
    c = (a % N + 1) * (N + 2) + a // N + 1
    return torch.where(none, torch.zeros_like(c), c).to(torch.int32)


def run(boards, ply=150):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(boards)
    tracked, plain = elf_amd.GoEngine(N, boards, 0, track_placed=True), elf_amd.GoEngine(N, boards, 0)
    for _ in range(ply - 1):
        mv = random_moves(tracked, gen)
        assert torch.equal(tracked.forward(None, mv), plain.forward(None, mv))
    out_df = torch.empty((boards, elf_amd.NUM_DF_PLANES, N, N), dtype=torch.float32, device="cuda")
    out_agz = torch.empty((boards, elf_amd.NUM_AGZ_PLANES, N, N), dtype=torch.float32, device="cuda")
    d4 = torch.arange(boards, dtype=torch.int32, device="cuda") % 8
    t_df, t_agz, t_ft, t_fp = [], [], [], []
    for rep in range(REPS + WARM):
        dt_a, _ = timed(lambda: tracked.extract_agz(d4=d4, out=out_agz))
        dt_d, _ = timed(lambda: tracked.extract_df(d4=d4, out=out_df))
        if rep >= WARM:
            t_df.append(dt_d)
            t_agz.append(dt_a)
    stones = float((out_df[:, 7].sum() + out_df[:, 8].sum()) / boards)
    for rep in range(REPS + WARM):
        mv = random_moves(tracked, gen)
        dt_p, ok_p = timed(lambda: plain.forward(None, mv))
        dt_t, ok_t = timed(lambda: tracked.forward(None, mv))
        assert torch.equal(ok_p, ok_t)
        if rep >= WARM:
            t_ft.append(dt_t)
            t_fp.append(dt_p)
    assert torch.equal(tracked.info(), plain.info())
    tracked.close()
    plain.close()

    def extract(times, planes):
        s = spread(times)
        row_bytes = planes * N * N * 4
        return dict(us_per_call=spread([t * 1e6 for t in times]), rows_per_s=boards / s["median"], bytes_written_per_s=boards * row_bytes / s["median"],
                    row_bytes=row_bytes, write_rate_over_hbm_peak=boards * row_bytes / s["median"] / HBM_PEAK)

    res = dict(boards=boards, ply=ply, reps=REPS, stones_per_board=stones, extract_df=extract(t_df, elf_amd.NUM_DF_PLANES),
               extract_agz_f32=extract(t_agz, elf_amd.NUM_AGZ_PLANES),
               forward_tracked_us=spread([t * 1e6 for t in t_ft]), forward_plain_us=spread([t * 1e6 for t in t_fp]))
    res["extract_df"]["bytes_rate_over_extract_agz"] = res["extract_df"]["bytes_written_per_s"] / res["extract_agz_f32"]["bytes_written_per_s"]
    res["extract_df"]["time_over_extract_agz"] = res["extract_df"]["us_per_call"]["median"] / res["extract_agz_f32"]["us_per_call"]["median"]
    res["forward_tracked_over_plain"] = res["forward_tracked_us"]["median"] / res["forward_plain_us"]["median"]
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "df_bench.json")
    res = dict(device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, boards_4096=run(4096), boards_16384=run(16384))
    text = json.dumps(res, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
