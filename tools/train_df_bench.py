"""GPU: the replay loader's DarkForest rows beside its AGZ rows, in one process on the same draws.

Two ReplayLoaders (feature_format "f32_nchw" and "df_f32_nchw", keep_states off) hold the same 19x19 records (uniformly random
legal play on the device engine, one policy and one value per ply).  Every repetition draws 16 batches of 2048 samples once
(elftrain_draw) and extracts them with both loaders, alternating -- k_replay_extract against k_replay_extract_df, one launch of
32 768 samples each.  Times are device events around the extraction, after a warm-up; medians of 12.  Reported per format:
samples per second, bytes per `s` row, TB/s of `s` written; and the DarkForest time over the AGZ time.  The stand-alone
extractors' figures (profiles/df_bench.json: extract_df beside extract_agz on boards held in engine slots) are quoted beside
them when that file is there.  Writes profiles/train_df_bench.json (or the path given as the first argument) and prints it."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import elf_amd

REPS, WARM = 12, 2
N, RECORDS, PLIES, BATCH, BATCHES = 19, 256, 320, 2048, 16
HBM_PEAK = 8.0e12   # bytes per second (MI355X)


def random_games(records, plies):
    """-> uint16 [records, plies] reference Coords: one uniformly random legal point per ply (pass where there is none)"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4242)
    eng = elf_amd.GoEngine(N, records, 0)
    out = torch.zeros((records, plies), dtype=torch.int32, device="cuda")
    for t in range(plies):
        legal = eng.legal_mask()[:, :-1].to(torch.float32)
        none = legal.sum(dim=1) == 0
        legal[none, 0] = 1
        a = torch.multinomial(legal, 1, generator=gen).squeeze(1)
        c = torch.where(none, torch.zeros_like(a), (a % N + 1) * (N + 2) + a // N + 1).to(torch.int32)
        eng.forward(None, c)
        out[:, t] = c
    eng.close()
    return out.cpu().numpy().astype(np.uint16)


def spread(v):
    v = sorted(v)
    return dict(min=v[0], median=v[len(v) // 2], max=v[-1])


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "train_df_bench.json")
    moves = random_games(RECORDS, PLIES)
    rng = np.random.default_rng(7)
    P = (N + 2) ** 2
    kinds = ("f32_nchw", "df_f32_nchw")
    ld = {k: elf_amd.ReplayLoader(board_size=N, capacity=RECORDS, batchsize=BATCH, num_future_actions=3, seed=1234, feature_format=k,
                                  batches_per_launch=BATCHES) for k in kinds}
    for r in range(RECORDS):
        pol = rng.integers(0, 256, (PLIES, P), dtype=np.uint8)
        pol[:, 0] |= 1
        rec = dict(moves=moves[r], reward=float(rng.choice([-1.0, 1.0])), black_ver=r, policies=pol,
                   values=np.tanh(rng.standard_normal(PLIES)).astype(np.float32))
        for k in kinds:
            ld[k].put(r, rec)
    B = BATCH * BATCHES
    out = {k: ld[k]._alloc(B) for k in kinds}
    d = ld[kinds[0]]._draw
    times = {k: [] for k in kinds}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(REPS + WARM):
        src = ld[kinds[0]]
        assert src.L.elftrain_draw(src._h, B, 3, C.c_void_p(d[0].data_ptr()), C.c_void_p(d[1].data_ptr()), C.c_void_p(d[2].data_ptr()), src._stream()) == 0
        for k in (kinds if rep % 2 == 0 else kinds[::-1]):
            a.record()
            ld[k].extract(d[0, :B], d[1, :B], d[2, :B], out=out[k])
            b.record()
            b.synchronize()
            if rep >= WARM:
                times[k].append(a.elapsed_time(b) * 1e-3)
        for f in ("move_idx", "aug_code", "offline_a", "winner"):
            assert torch.equal(out[kinds[0]][f], out[kinds[1]][f]), f
    res = dict(device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, board_size=N, records=RECORDS, plies=PLIES,
               samples_per_launch=B, batches_per_launch=BATCHES, batch=BATCH, keep_states=False, reps=REPS,
               mean_move_idx=float(out[kinds[0]]["move_idx"].float().mean()))
    for k in kinds:
        s = spread(times[k])
        row = ld[k].num_planes * N * N * 4
        res[k] = dict(ms_per_launch=spread([t * 1e3 for t in times[k]]), samples_per_s=B / s["median"], s_row_bytes=row,
                      s_bytes_written_per_s=B * row / s["median"], s_write_rate_over_hbm_peak=B * row / s["median"] / HBM_PEAK)
        ld[k].close()
    df, agz = res["df_f32_nchw"], res["f32_nchw"]
    res["df_over_agz"] = dict(time=df["ms_per_launch"]["median"] / agz["ms_per_launch"]["median"], s_row_bytes=df["s_row_bytes"] / agz["s_row_bytes"],
                              s_bytes_rate=df["s_bytes_written_per_s"] / agz["s_bytes_written_per_s"])
    alone = os.path.join(ROOT, "profiles", "df_bench.json")
    if os.path.exists(alone):
        sa = json.load(open(alone))["boards_16384"]["extract_df"]
        res["stand_alone_extractors"] = dict(source="profiles/df_bench.json, 16 384 boards in engine slots",
                                             bytes_rate_over_extract_agz=sa["bytes_rate_over_extract_agz"], time_over_extract_agz=sa["time_over_extract_agz"])
    text = json.dumps(res, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
