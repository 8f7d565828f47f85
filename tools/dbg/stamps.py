"""Phase stamps (wall_clock64, 100 MHz) of the merge kernel [0..6] and workgroup 0 of the single-launch kernel [8..14].

``--census`` (a library built with ``-DICEM_WAVE_CENSUS``: ``ICEM_WAVE_CENSUS=1 python -m icem_amd.build``; a product library
leaves the words zero): where the waves of the first and the last workgroup of the last merge-prologue launch ran (HW_ID:
SIMD, CU, SE), how the selection wave's time into the prologue's first barrier splits, and where between "mapped" (stamp 10)
and "rolled out" (stamp 12) wave 0 starts its first model step (the set-up from the start observation lies in front of it:
hoisted ahead of the barriers for the fp16-plane tile, tile_scales.h) -- words [16..63] of the buffer."""
import sys, os, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from icem_amd import IcemConfig, IcemPlanner, DeviceSyntheticModel, halfcheetah_env
from icem_amd import _lib as L
from icem_amd import _lib as _LENV  # noqa: E402
_LENV.follow_environment()   # ICEM_<NAME> variables (incl. ICEM_TILE_ARITH) are mapped per planner: the library reads no environment
env = halfcheetah_env(17)
CENSUS = "--census" in sys.argv
argv = [a for a in sys.argv if a != "--census"]
N = int(argv[1]) if len(argv) > 1 else 4096
ITERS = int(argv[2]) if len(argv) > 2 else 1
model = DeviceSyntheticModel.make(17, 6)
pl = IcemPlanner(IcemConfig(horizon=30, act_dim=6, num_traj=N, opt_iters=ITERS, dtype="f32", seed=1), env.action_space.low, env.action_space.high)
pl.set_model(model.kind, model.A, model.B)
c = env.cost_spec
pl.set_cost(c.ctrl_weight, c.lin_idx, c.lin_weight, c.flip_idx, c.flip_penalty, c.flip_thresh)
pl.reset()
obs = 0.1 * np.random.RandomState(0).randn(17)
dbg = torch.zeros(64, dtype=torch.int64, device="cuda")   # 16 stamps + the census words (a census build writes them whatever the flag)
L.check(pl.lib.icem_debug_stamps(pl._h, dbg.data_ptr()))
for _ in range(5):
    pl.plan_step(obs)
torch.cuda.synchronize()
acc = np.zeros(16)
pro = np.zeros(2)
gap = 0.0
R = 20
cen_t = np.zeros((2, 11))     # per census workgroup: first instruction, keys loaded, selected, waves 0..6 at the barrier, met
first_step = np.zeros(4)      # workgroup 0 of the last merge-prologue launch: mapped, behind the barrier, first model step, rolled out
placements = [dict(), dict()]  # (SIMD of wave 0..6) -> number of steps it was seen in
where = [None, None]
for _ in range(R):
    pl.plan_step(obs); torch.cuda.synchronize()
    raw = dbg.cpu().numpy()
    d = raw.astype(np.float64)
    if CENSUS:
        for g in range(2):
            c = raw[16 + 24 * g:16 + 24 * (g + 1)]
            if c[8] == 0:
                continue
            ids = [int(v) & 0xFFFFFFFF for v in c[:7]]
            simd = tuple((v >> 4) & 3 for v in ids)
            placements[g][simd] = placements[g].get(simd, 0) + 1
            where[g] = sorted({((v >> 13) & 7, (v >> 8) & 15) for v in ids})   # (SE, CU)
            cen_t[g] += (np.concatenate([c[9:12], c[12:19], c[19:20]]) - c[8]) / 100.0 / R
            if g == 0 and c[20] != 0:   # (word 20: wave 0 of workgroup 0 in front of its first model step)
                first_step += np.array([d[10] - d[8], d[11] - d[8], c[20] - d[8], d[12] - d[8]]) / 100.0 / R
    acc[:7] += (d[:7] - d[0]) / 100.0
    acc[8:15] += (d[8:15] - d[8]) / 100.0
    gap += (d[0] - d[14]) / 100.0 / R   # (slot 15 itself is a stamp of the prologue: pro, below)
    pro += np.array([d[15] - d[8], d[7] - d[8]]) / 100.0 / R
acc /= R
print("merge  [us from kernel start]: lists loaded %.2f | keep merged %.2f | threshold+compact %.2f | selected %.2f | gather+refit %.2f | end %.2f" % tuple(acc[1:7]))
# (stamp 12, "wave 0 rolled out", exists only on the Tile16 path; the Tile4 path of small populations goes straight to 13)
print("single [us from kernel start]: staged %.2f | sampled %.2f | tile->HBM issued %.2f | rolled out %.2f | end %.2f"
      % (acc[9], acc[10], acc[11], acc[13], acc[14]))
print("       wave 0 through its 30 steps (stamp 12, in front of the top-K push and the list): %.2f" % acc[12])
print("gap end(single, wg 0) -> start(merge): %.2f us" % gap)
if ITERS > 1:   # the prologue's own stamps 5 / 6, which the last merge overwrites: the lists form repeats them in slots 15 / 7
    print("prologue of the last single launch [us from kernel start]: selection and sampling waves met %.2f | gather + refit done %.2f"
          % (pro[0], pro[1]))
print("(with ITERS > 1 the stamps are those of the LAST iteration: the single-launch kernel then carries the previous merge in its prologue"
      " and 'sampled' includes selection + gather + refit + affine map)")
if CENSUS:
    if first_step[2] > 0:
        print("wave 0 of workgroup 0 [us from kernel start]: mapped %.2f | behind the last barrier %.2f | first model step %.2f | rolled out %.2f"
              "  (barrier to first step %.2f, the steps %.2f)"
              % (*first_step, first_step[2] - first_step[1], first_step[3] - first_step[2]))
    for g, name in enumerate(("first", "last")):
        if not placements[g]:
            print("census, %s workgroup: nothing recorded (a library without -DICEM_WAVE_CENSUS, or no merge-prologue launch)" % name)
            continue
        t = cen_t[g]
        after = np.where(t[3:10] >= t[2], t[3:10] - t[2], np.inf)
        selw = int(np.argmin(after))   # the wave whose barrier stamp follows "selected"
        print("census, %s workgroup of the last merge-prologue launch, (SE, CU) %s:" % (name, where[g]))
        for simd, cnt in sorted(placements[g].items(), key=lambda kv: -kv[1]):
            alone = [w for w in range(7) if simd.count(simd[w]) == 1]
            print("   SIMD of waves 0..6: %s  in %d of %d steps; alone on its SIMD: wave %s" % (list(simd), cnt, R, alone))
        print("   selection wave (wave %d) [us from the workgroup's first stamp]: first instruction %.2f | keys loaded %.2f | selected %.2f"
              % (selw, t[0], t[1], t[2]))
        print("   waves 0..6 at the first barrier: %s | wave 0 behind it %.2f" % (" ".join("%.2f" % v for v in t[3:10]), t[10]))
