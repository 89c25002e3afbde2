"""Federated averaging of the MaPLe trainables across clients, one or more clients per GPU.

Reference (trainers/maple_fed.py):
  * check_weights_valid (:317-325)  per-key isnan/isinf scan of a client's state dict, host sync per key;
  * safe_average_weights (:309-315) per key: stack(float) -> nan_to_num -> mean(0) -> .half(), over the
    clients whose weights were valid (:271-277); all invalid -> round skipped (:288-290);
  * broadcast_weights (:327-339)    load_state_dict + drop SGD momentum + rebuild the LR schedule.

MI355X form: the N clients are spread over the ranks in contiguous blocks (rank r trains clients
r*C .. r*C + C - 1 one after another, C = N / world; C = 1 is one client per GPU).  For every client
  1. one kernel scans its flat trainable buffers (mf_nonfinite_flag) -> device int flag;
  2. its buffers are packed into one fp32 bucket [fp16 trainables | fp32 trainables | vote] with its
     validity vote (an invalid client packs zeros and vote 0; mf_fedavg_pack);
then FedAvgExchange moves every rank's buckets over RCCL (xGMI), asynchronously, so the caller overlaps
the collective with the last client's last local test() (trainers/maple.py:646), and finally
  3. every bucket unpacks mean = sum / n_valid rounded to fp16 into its client's trainables
     (mf_fedavg_unpack): the reference's `.half()` of every key, incl. fp32 LN params, deep prompts and
     logit_scale.

Two exchange modes (FED.AGGREGATION in the trainer config):
  * "ordered" (default): a sharded client-ordered sum.  Every bucket (57 MB per client at J=9, padded to
    a multiple of the world size W) is cut into W shards; one all_to_all hands rank r shard r of every
    client ([source rank][local client] = global client order), rank r sums its shard over the N clients
    in client order on the device (mf_fedavg_reduce_ordered), and one all_gather returns every summed
    shard to every rank.  Each rank moves 2(W-1)/W of C buckets, the traffic of a ring all-reduce, but
    the fp32 summation order is the reference's torch.stack(...) order, so the fp16 result is
    bit-identical to safe_average_weights at any world size (CPU-torch mean semantics: sum then divide,
    which tests/golden/fedavg.npz pins).  On a GPU the chain runs on a side stream (all_to_all -> reduce
    -> all_gather), so start() returns at once and the caller's next kernels run under it; under gloo (the
    world-size 2 / 3 / 8 CPU tests) the same _ordered_chain runs with host waits, so those tests cover its
    collective order and arithmetic -- not the RCCL stream dependencies, nor the start() / finish() overlap
    with caller kernels, which only an RCCL run with more than one GPU exercises (the driver's 8-GPU bench).
  * "allreduce": the rank's buckets summed in client order, then one RCCL all_reduce(SUM).  The same
    traffic, but RCCL's ring order changes the fp32 summation order per chunk; with three or more ranks the
    fp16-rounded result can differ from the reference's in the last fp16 bit of rare elements.
A client that fails after its bucket was packed (its last test() raising, after the exchange started) is
still excluded, as the reference's `continue` excludes it (trainers/maple_fed.py:262-265): finish() agrees
on such late failures with one 4-byte all_reduce and, when there is one, re-packs every local bucket
(failed ones with vote 0; the weights are untouched until unpack) and exchanges again.
Frozen tensors are bit-identical across clients, so leaving them out of the bucket is result-preserving
(an fp32 mean of identical fp16 values is exact).  With world_size 1 (or no process
group) the same kernels run with no collective.

Sample-weighted FedAvg (McMahan et al., AISTATS 2017; FED.CLIENT_WEIGHTS, off by default): a bucket built with
weight=w packs [w * trainables | w | vote] (mf_fedavg_pack_weighted), the exchange sums the n + 2 floats exactly as
it sums the n + 1 of the plain layout, and unpack divides by the summed weights (mf_fedavg_unpack_weighted).  The
fp32 products are rounded in the pack kernel and summed in client order, so the "ordered" result equals the torch
expression acc = w0*x0; acc += wc*xc ...; (acc / sum w).half() bit for bit at any world size.

FedOpt server optimizers (FED.SERVER_OPT, off by default): FedAvgM (Hsu et al., 2019) and FedAdagrad / FedAdam /
FedYogi (Reddi et al., ICLR 2021, Algorithm 2).  The global weights are fp16, and a server step
eta * m / (sqrt(v) + tau) with a small eta moves hardly any fp16 weight, so ServerOptimizer keeps an fp32 master
copy x of the trainables with the moments m and v, and the clients receive fp16(x).  The step runs in the kernel
that otherwise turns the summed bucket into weights (mf_fedopt_step in mf_fedavg_unpack's place: no host
synchronisation, no extra pass): the round's (weighted) mean is the pseudo-gradient's target, delta = mean - x.  One
ServerOptimizer per process serves all of the rank's buckets; the first unpack() after the rank's packs applies the
step and writes that client, the others receive the same fp16(x) (mf_fedopt_deliver), so the step runs exactly once
per completed exchange -- also after a late-failure re-exchange, which packs again before any unpack.  Every rank
applies the step to the same total (each holds the whole summed bucket after either exchange mode, and at world
size 1) with the same kernel, so the replicated states stay bit-identical across the ranks without a further
collective.  A round without a valid client leaves x, m, v untouched.  An x outside the fp16 range is delivered as
+-inf, and the next round's validity scan then excludes every client.

Robust aggregation (FED.ROBUST_AGG, off by default): the coordinate-wise median and the coordinate-wise trimmed mean
of Yin, Chen, Ramchandran and Bartlett (ICML 2018), so that one client returning finite but wrong weights (a diverged
local run, a corrupted shard) cannot move a global weight further than the honest clients' values reach.  A bucket
built with robust="median" | "trimmed_mean" packs the weighted layout at weight 1, [trainables | 1 | 1], and an invalid
client packs NaNs -- "absent" -- instead of zeros (mf_fedavg_pack_robust).  The "ordered" exchange is unchanged: rank r
still receives shard r of every client's bucket in client order, which is exactly what a per-coordinate order
statistic needs, and mf_fedavg_reduce_trimmed runs where mf_fedavg_reduce_ordered does: per coordinate it sorts the
present values, drops trim_k at either end (as many as leave something; the median is a trim nobody reaches), sums
the rest in ascending order and divides by their number.  At the vote element it writes the number of present
clients instead, so the reduced bucket reads [statistic | 1 | n_valid] and the weighted unpack, the server step and
n_valid() consume it as they are; with a server optimizer the statistic is the pseudo-gradient's target.  A sum in
sorted order depends on neither the client order, the world size nor the clients per rank, so the fp32 statistic
equals a single-process restatement bit for bit at any layout (tests/test_fedavg_robust_dist.py).  One process runs
the same kernel over its buckets staged contiguously, also for a single client: it is what turns the absence marks
into a zero vote.  Not combined with "allreduce" (a sum has lost the per-client values) or with client weights (a
weighted median is another statistic).

Multi-Krum (robust="multi_krum", krum_f=1, krum_m=0; FED.ROBUST_AGG multi_krum, FED.KRUM_F, FED.KRUM_M): Blanchard, El
Mhamdi, Guerraoui and Stainer (NeurIPS 2017), keeping the m best as El Mhamdi, Guerraoui and Rouault do (ICML 2018).  A
coordinate-wise statistic still mixes every client into every coordinate; Multi-Krum drops whole clients.  The bucket
and the image are the robust ones, and three kernels run in the trimmed reduce's place: mf_krum_pairwise forms the fp64
squared distances D[i][j] of this rank's shard of every client (an absent client's NaNs make its row, column and
diagonal NaN), one all_gather hands every rank the W partial matrices (W * N^2 doubles), mf_krum_select adds them in
rank order, scores every present client by the sum of its p - f' - 2 smallest distances and keeps the m' best (f' and
m' degrade with the number p of present clients, as the trim does), and mf_fedavg_reduce_selected averages the kept
clients in client order, writing p at the vote element, so the reduced bucket again reads [statistic | 1 | p].  Given
the selection the statistic depends on no layout; the distances' last fp64 bits do (the shard boundaries move), so two
layouts can select differently only where two scores lie within 2 n 2^-53 of each other.  All ranks
add the same parts in the same order and always agree.  krum_m = 1 is Krum; krum_m = 0 keeps all but f'.  Every
exclusion of the robust aggregation holds: not with "allreduce", client weights, dp_std, topk or dyn; dp_clip, int8,
the server optimizers and FedProx combine as with the median.

DP-FedAvg (FedAvgBucket dp_clip / FedAvgExchange dp_std; FED.DP_CLIP and FED.DP_NOISE_MULTIPLIER, off by default):
user-level differential privacy as McMahan, Ramage, Talwar and Zhang define it (ICLR 2018; Geyer et al. 2017).  Each
client's update Delta_k = w_k - g against the round's starting weights g (the bucket's global copy) is clipped to the L2
bound S, Gaussian noise of standard deviation z * S is added to the sum, and dp_epsilon reports the (eps, delta) this
buys.  The clipping half alone bounds a client that scales its update (Sun et al., 2019), which no per-coordinate
statistic does, so dp_clip combines with client weights, the robust aggregation, the server optimizer and FedProx.
pack() runs mf_dp_update_scale (norm = ||Delta_k||_2 in two launches, s_k = S / norm when norm > S, else exactly 1; it
stays on the device) and then mf_fedavg_pack_clipped, which packs g + s_k * Delta_k in the bucket's layout: the bucket
keeps holding weights, because the sum over the m valid clients is m * g + sum_k s_k Delta_k and every reduce, unpack
and server step downstream consumes it unchanged -- no second layout, no extra traffic.  s_k >= 1 selects the weight
itself, so a bound nobody reaches gives the bits of the plain exchange.  The noise is counter-based: its value at global
coordinate i is a function of (seed, round, i) alone (Philox4x32-10 -> Box-Muller, mf_dp_add_noise), so in the sharded
chain rank r noises its own shard [r * S, r * S + S) between the reduce and the all_gather, "allreduce" noises the
whole sum on every rank after the all_reduce, one process after its local sum, and every layout ends with the same
bits; only the n summed coordinates are noised, never the weight sum, the vote or the padding.  The exchange counts
its rounds (finish() advances the counter once; a late-failure re-exchange reuses the round's value, and only that
second sum is ever unpacked) and carries {round, seed} in its state_dict, so a resumed run never reuses a noise
stream.  The noise needs the plain mean: with client weights the sensitivity would be w_k S / sum w, and an order
statistic has another one.

int8 compression of the uplink with error feedback (FedAvgBucket compress="int8"; FED.COMPRESS, off by default): the
update u = (w_k - g) + e against the bucket's global copy is quantised to 8 bits per coordinate with one fp32 scale per
block of 256 coordinates, rounded to nearest or stochastically (QSGD, Alistarh et al., NeurIPS 2017; the rounding bits
are a function of (seed, round, client, coordinate) alone, Philox again), and the rounding error e' = u - scale * q
stays with the client as next round's residual (Seide et al. 2014; Karimireddy et al., ICML 2019).  pack() runs
mf_compress_quantize, which writes the codes, the scales and a {weight, vote} tail straight into the exchange's uint8
send image [destination rank][client][chunk], chunk = S + S / 64 + 8 bytes for a shard of S coordinates (S is then a
multiple of 256): 1 + 1/64 bytes per coordinate where the fp32 bucket moves 4.  In the sharded "ordered" chain the
all_to_all moves that image and the receiver rebuilds, with mf_compress_decode and the global copy every rank holds, the
fp32 image g + scale * q of its shard of every client -- exactly what the pack kernels would have sent for those weights
-- so the ordered or trimmed reduce, the all_gather (the downlink stays fp32), the unpack and the server step run
unchanged, and client weights, the robust aggregation, the server optimizers and FedProx combine with it as they are.
One process and "allreduce" decode each bucket locally right away and then run as before: the arithmetic of
compression, none of its savings.  pack() reads e and writes e' to a second buffer; unpack() swaps the two, once per
round and only for a client that did not fail, so a late-failure re-pack reads the same e, weights, global copy and
round, reproduces the same codes, and the residual is applied once; an invalid or failed client sends nothing (codes,
scales and vote 0) and keeps its residual.  Not combined with dp_clip / dp_std: a quantised, fed-back update no longer
has an L2 norm within the bound.

Top-k sparsification of the uplink with error feedback (FedAvgBucket compress="topk", compress_k=8; FED.COMPRESS topk,
FED.COMPRESS_TOPK): the same update u, the same residual and its two-buffer commit, the same send image and the same
places for the decode, but from every block of 256 coordinates only the k of largest magnitude travel, as (uint8 index
within the block, fp32 value), a tie going to the lower index (Aji & Heafield, EMNLP 2017; Stich et al., NeurIPS 2018;
Lin et al., ICLR 2018; Sattler et al. 2019): chunk = 4 nb k + 4 ceil(nb k / 4) + 8 bytes for a shard of nb blocks, 40
bytes per block at k = 8 where the fp32 bucket moves 1024 and int8 moves 260.  Nothing is rounded: a coordinate's update
is sent whole (e' = 0) or stays whole in the residual (e' = u), and the receiver adds the sent value, or +0, to the
global copy (mf_topk_select, mf_topk_decode).  The blocks start at coordinate 0 whatever the world size, so every layout
gives the same bits.  Not with stochastic rounding (there is nothing to round), not with the robust aggregation (most
coordinates of every client decode to g itself, so a median returns g unless half the clients kept the coordinate), and,
as int8, not with dp_clip / dp_std or dyn.  The two codecs are one encode and one decode kernel body with a codec each
(csrc/compress.hip) behind one pair of wrappers (ops.py), and FedAvgExchange's constructor is the one place here that
tells them apart: it keeps the chunk size and the two kernels with the arguments of their own, and pack(),
decode_local() and the sharded chain make one call each.

FedDyn (FedAvgBucket dyn= / FedDynState; FED.DYN_ALPHA, off by default): the dynamic regularisation of Acar, Zhao, Matas
Navarro, Mattina, Whatmough and Saligrama (ICLR 2021), which makes the clients' local optima agree with the global one
where FedProx only pulls them towards the last global model.  Client k minimises L_k(w) - <lam_k, w> + (alpha / 2)
||w - g||^2: the captured step's SGD launch reads the bucket's global copy, as under FedProx, and the client's fp32
correction lam_k besides (engine.set_dynamic, mf_optimizer_step_dyn).  The round's end moves no extra byte -- the bucket,
the exchange and the reduce are the plain ones -- and runs in the one kernel that would otherwise unpack the mean
(mf_feddyn_step in mf_fedavg_unpack's place): lam_k = lam_k - alpha * (w_k - g) for a client that took part, the server's
h = h - alpha * (m / N) * (mean - g) over the m voting of the N clients, and every client receives
fp16(mean - h / alpha).  One FedDynState per process holds h, fp32 of the bucket's size, replicated as the FedOpt state
is: every rank steps it on the same summed bucket with the same kernel.  The first unpack() after the rank's packs
steps h and writes that client; the others (mf_feddyn_deliver) read the stepped h and the same bucket and so recompute
the same weights, each updating its own lam_k: no fp32 copy of the model is kept.  An invalid, failed or late-failed
client (the bucket's device flag) keeps its lam_k, the paper's rule for a device that did not take part, and its
absence reaches h through m / N; a round without a valid client leaves h and every lam_k untouched.  h is the mean of
the lam_k by construction only while the server sees the clients' own weights in a plain mean, so dyn is not combined
with client weights, the robust aggregation, dp_clip, compress or a server optimizer; both exchange modes are allowed.
"""
from __future__ import annotations

import math
from typing import Iterable, List, Optional, Sequence

import torch
import torch.distributed as dist

from . import ops

MODES = ("ordered", "allreduce")
ROBUST = ("median", "trimmed_mean", "multi_krum")
MEDIAN_TRIM = ops.MEDIAN_TRIM  # a trim no client count reaches: the trimmed reduce degrades it to the median
KRUM_TRIM = -1  # robust_trim's value for "multi_krum": the robust layout, no trimmed reduce
COMPRESS = ("int8", "topk")
TOPK_MAX = ops.TOPK_MAX  # entries kept per block of COMPRESS_BLOCK coordinates, at most
COMPRESS_ROUNDINGS = tuple(ops.COMPRESS_ROUNDINGS)
COMPRESS_BLOCK = ops.COMPRESS_BLOCK  # coordinates per quantisation block; a compressed shard is a multiple of it


def dp_epsilon(z: float, rounds: int, delta: float) -> float:
    """The epsilon of `rounds` Gaussian mechanisms of noise multiplier z (standard deviation z * S on a sum of L2
    sensitivity S), every client taking part in every round, at `delta`, by Renyi-DP composition (Mironov, CSF 2017):
    each round is (alpha, alpha / (2 z^2))-RDP, T rounds add up, and the conversion eps = T alpha / (2 z^2) +
    ln(1 / delta) / (alpha - 1) is least at alpha = 1 + z sqrt(2 ln(1 / delta) / T), which gives the closed form
    eps = T / (2 z^2) + sqrt(2 T ln(1 / delta)) / z.  z = 0 gives inf; no round gives 0."""
    z, delta = float(z), float(delta)
    if isinstance(rounds, bool) or int(rounds) != rounds or rounds < 0:
        raise ValueError(f"dp_epsilon: rounds {rounds!r}: an integer >= 0")
    if math.isnan(z) or z < 0.0:
        raise ValueError(f"dp_epsilon: noise multiplier {z}: >= 0")
    if not 0.0 < delta < 1.0:
        raise ValueError(f"dp_epsilon: delta {delta}: in (0, 1)")
    if rounds == 0:
        return 0.0
    if z == 0.0:
        return math.inf
    t = float(rounds)
    return t / (2.0 * z * z) + math.sqrt(2.0 * t * math.log(1.0 / delta)) / z


def robust_trim(robust: Optional[str], trim_k: int, mode: str = "ordered", weighted: bool = False) -> Optional[int]:
    """The trim the reduce kernel is called with (None: no robust aggregation; KRUM_TRIM for "multi_krum", which has
    a reduce of its own).  ValueError for an unknown name, the "allreduce" mode, client weights, or trim_k < 1 for
    "trimmed_mean"."""
    if robust is None:
        return None
    if robust not in ROBUST:
        hint = ' (Krum is "multi_krum" with krum_m = 1)' if robust == "krum" else ""
        raise ValueError(f"robust aggregation {robust!r}: None or one of {ROBUST}{hint}")
    if mode != "ordered":
        raise ValueError(f'robust aggregation needs mode "ordered" (got {mode!r}): a sum has lost the per-client values')
    if weighted:
        raise ValueError("robust aggregation with a client weight: a weighted median is a different statistic")
    if robust == "median":
        return MEDIAN_TRIM
    if robust == "multi_krum":
        return KRUM_TRIM
    if isinstance(trim_k, bool) or not isinstance(trim_k, int) or not 1 <= trim_k <= MEDIAN_TRIM:
        raise ValueError(f"trimmed_mean trim_k {trim_k!r}: an integer >= 1")
    return trim_k


def check_krum(krum_f, krum_m):
    """Multi-Krum's f (clients tolerated as wrong) and m (clients kept; 0: all but f): integers >= 0."""
    for label, v in (("krum_f", krum_f), ("krum_m", krum_m)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 31:
            raise ValueError(f"multi_krum {label} {v!r}: an integer >= 0")
    return krum_f, krum_m


class FederatedAbort(RuntimeError):
    """Raised on every rank when one rank stops the run (FedAvgExchange.finish(abort=True))."""


class _HipKernels:
    """The device kernels FedAvgBucket drives (libmapfed.so)."""
    nonfinite_flag = staticmethod(ops.nonfinite_flag)
    fedavg_pack = staticmethod(ops.fedavg_pack)
    fedavg_unpack = staticmethod(ops.fedavg_unpack)
    fedavg_pack_weighted = staticmethod(ops.fedavg_pack_weighted)
    fedavg_unpack_weighted = staticmethod(ops.fedavg_unpack_weighted)
    fedavg_reduce_ordered = staticmethod(ops.fedavg_reduce_ordered)
    fedopt_step = staticmethod(ops.fedopt_step)
    fedopt_deliver = staticmethod(ops.fedopt_deliver)
    fedavg_pack_robust = staticmethod(ops.fedavg_pack_robust)
    fedavg_reduce_trimmed = staticmethod(ops.fedavg_reduce_trimmed)
    krum_ws_bytes = staticmethod(ops.krum_ws_bytes)
    krum_pairwise = staticmethod(ops.krum_pairwise)
    krum_select = staticmethod(ops.krum_select)
    fedavg_reduce_selected = staticmethod(ops.fedavg_reduce_selected)
    dp_update_ws_floats = staticmethod(ops.dp_update_ws_floats)
    dp_update_scale = staticmethod(ops.dp_update_scale)
    fedavg_pack_clipped = staticmethod(ops.fedavg_pack_clipped)
    dp_add_noise = staticmethod(ops.dp_add_noise)
    compress_chunk_bytes = staticmethod(ops.compress_chunk_bytes)
    compress_quantize = staticmethod(ops.compress_quantize)
    compress_decode = staticmethod(ops.compress_decode)
    topk_chunk_bytes = staticmethod(ops.topk_chunk_bytes)
    topk_select = staticmethod(ops.topk_select)
    topk_decode = staticmethod(ops.topk_decode)
    feddyn_step = staticmethod(ops.feddyn_step)
    feddyn_deliver = staticmethod(ops.feddyn_deliver)


SERVER_OPTS = ("fedavgm", "fedadagrad", "fedadam", "fedyogi")


class ServerOptimizer:
    """The FedOpt server state of one process, shared by the rank's buckets (module docstring): the fp32 master copy
    x of the trainables ([fp16 trainables | fp32 trainables], the bucket's order), the first moment m and, for the
    adaptive optimizers, the second moment v.  x = float(global copy), m = 0, v = tau * tau (an fp32 product;
    Reddi et al. require v_{-1} >= tau^2) until a round completes.  FedAvgM has no v."""

    def __init__(self, name: str, engine, lr: float = 1.0, beta1: float = 0.9, beta2: float = 0.99,
                 tau: float = 1e-3):
        if name not in SERVER_OPTS:
            raise ValueError(f"server optimizer {name!r}: one of {SERVER_OPTS}")
        lr, beta1, beta2, tau = float(lr), float(beta1), float(beta2), float(tau)
        if not math.isfinite(lr) or lr < 0.0:
            raise ValueError(f"server learning rate {lr}: finite and >= 0")
        for label, b in (("momentum (beta1)", beta1), ("beta2", beta2)):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"server {label} {b}: in [0, 1)")
        self.adaptive = name != "fedavgm"
        if not math.isfinite(tau) or (self.adaptive and tau <= 0.0):
            raise ValueError(f"server tau {tau}: finite and > 0")
        self.name, self.lr, self.beta1, self.beta2, self.tau = name, lr, beta1, beta2, tau
        # engine: what FedAvgBucket needs (n16, n32, flat16, flat32), holding the initial global weights
        self.n16, self.n32 = engine.n16, engine.n32
        n, dev = self.n16 + self.n32, engine.flat16.device
        self.x = torch.empty(n, device=dev, dtype=torch.float32)
        self.m = torch.empty(n, device=dev, dtype=torch.float32)
        self.v = torch.empty(n, device=dev, dtype=torch.float32) if self.adaptive else None
        self.pending = False  # a pack since the last step: the next unpack applies the step, the others deliver
        self._reset(engine.flat16, engine.flat32)

    def hyper(self) -> dict:
        return {"lr": self.lr, "beta1": self.beta1, "beta2": self.beta2, "tau": self.tau}

    def reset_from(self, bucket: "FedAvgBucket"):
        """Restart from a bucket's global copy: x = its fp32 value, m = 0, v = tau * tau."""
        if (bucket.e.n16, bucket.e.n32) != (self.n16, self.n32):
            raise ValueError("ServerOptimizer.reset_from: a bucket of another size")
        self._reset(bucket.global16, bucket.global32)

    def _reset(self, g16, g32):
        self.x[:self.n16].copy_(g16.detach())
        self.x[self.n16:].copy_(g32.detach())
        self.m.zero_()
        if self.v is not None:
            t = torch.tensor(self.tau, dtype=torch.float32)
            self.v.fill_(float(t * t))

    def state_dict(self) -> dict:
        """CPU tensors and plain numbers only (torch.load(..., weights_only=True) reads it)."""
        return {"name": self.name, "hyper": self.hyper(), "n16": self.n16, "n32": self.n32,
                "x": self.x.detach().cpu().clone(), "m": self.m.detach().cpu().clone(),
                "v": None if self.v is None else self.v.detach().cpu().clone()}

    def load_state_dict(self, sd: dict):
        """The moments and the master copy of a saved state; this optimizer's own hyper-parameters stay (they are
        the run's configuration).  ValueError for another optimizer or other sizes."""
        if sd.get("name") != self.name:
            raise ValueError(f"server optimizer state of {sd.get('name')!r}, this one is {self.name!r}")
        if (sd.get("n16"), sd.get("n32")) != (self.n16, self.n32):
            raise ValueError(f"server optimizer state of sizes {(sd.get('n16'), sd.get('n32'))}, "
                             f"this one has {(self.n16, self.n32)}")
        keys = ("x", "m") + (("v",) if self.adaptive else ())
        for k in keys:
            t = sd.get(k)
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != self.n16 + self.n32:
                raise ValueError(f"server optimizer state: {k!r} is not fp32 of {self.n16 + self.n32} elements")
        for k in keys:
            getattr(self, k).copy_(sd[k].reshape(-1))


class FedDynState:
    """FedDyn's server state of one process, shared by the rank's buckets (module docstring): h, the mean of the
    num_clients clients' corrections lam_k, fp32 zeros of n16 + n32 elements in the bucket's order until a round
    completes.  Each bucket keeps its own lam_k."""

    def __init__(self, alpha: float, engine, num_clients: int):
        alpha = float(alpha)
        if not math.isfinite(alpha) or alpha <= 0.0:
            raise ValueError(f"FedDyn alpha {alpha}: finite and > 0")
        if isinstance(num_clients, bool) or not isinstance(num_clients, int) or num_clients < 1:
            raise ValueError(f"FedDyn num_clients {num_clients!r}: an integer >= 1")
        self.alpha, self.num_clients = alpha, num_clients
        # engine: what FedAvgBucket needs (n16, n32, flat16)
        self.n16, self.n32 = engine.n16, engine.n32
        self.h = torch.zeros(self.n16 + self.n32, device=engine.flat16.device, dtype=torch.float32)
        self.pending = False  # a pack since the last step: the next unpack steps h, the others deliver

    def reset(self):
        self.h.zero_()

    def state_dict(self) -> dict:
        """CPU tensors and plain numbers only (torch.load(..., weights_only=True) reads it)."""
        return {"alpha": self.alpha, "num_clients": self.num_clients, "n16": self.n16, "n32": self.n32,
                "h": self.h.detach().cpu().clone()}

    def load_state_dict(self, sd: dict):
        """The h of a saved state; this state's own alpha and client count stay (they are the run's configuration).
        ValueError for other sizes."""
        if (sd.get("n16"), sd.get("n32")) != (self.n16, self.n32):
            raise ValueError(f"FedDyn state of sizes {(sd.get('n16'), sd.get('n32'))}, this one has "
                             f"{(self.n16, self.n32)}")
        t = sd.get("h")
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != self.n16 + self.n32:
            raise ValueError(f"FedDyn state: 'h' is not fp32 of {self.n16 + self.n32} elements")
        self.h.copy_(t.reshape(-1))


def resolve_client_weights(spec, sample_counts: Sequence[int], num_clients: int) -> Optional[List[float]]:
    """FED.CLIENT_WEIGHTS -> one FedAvg weight per client, or None for the unweighted mean.

    "uniform" -> None; "samples" -> sample_counts (each client's number of training samples) as floats; a list,
    a tuple or a comma-separated string -> those values.  ValueError for a wrong length, a weight that is
    non-finite or <= 0, or a sample count >= 2**24 (not exact in fp32, the bucket's number format)."""
    if isinstance(spec, str):
        name = spec.strip().lower()
        if name == "uniform":
            return None
        if name == "samples":
            counts = list(sample_counts)
            if len(counts) != num_clients:
                raise ValueError(f"FED.CLIENT_WEIGHTS samples: {len(counts)} sample counts for {num_clients} clients")
            for c in counts:
                if int(c) != c or c >= 2 ** 24:
                    raise ValueError(f"FED.CLIENT_WEIGHTS samples: a count of {c} is not exact in fp32 (>= 2**24) "
                                     "or not an integer; give explicit weights")
            vals = [float(c) for c in counts]
        else:
            try:
                vals = [float(v) for v in spec.split(",")]
            except ValueError:
                raise ValueError(f'FED.CLIENT_WEIGHTS {spec!r}: "uniform", "samples" or one weight per client') from None
    elif isinstance(spec, (list, tuple)):
        try:
            vals = [float(v) for v in spec]
        except (TypeError, ValueError):
            raise ValueError(f"FED.CLIENT_WEIGHTS {spec!r}: the weights must be numbers") from None
    else:
        raise ValueError(f'FED.CLIENT_WEIGHTS {spec!r}: "uniform", "samples" or one weight per client')
    if len(vals) != num_clients:
        raise ValueError(f"FED.CLIENT_WEIGHTS: {len(vals)} weights for {num_clients} clients")
    for v in vals:
        if not math.isfinite(v) or v <= 0.0:
            raise ValueError(f"FED.CLIENT_WEIGHTS: weight {v} is not finite and > 0")
    return vals


def _world(group) -> int:
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


class FedAvgBucket:
    """One client's bucket.  `engine` needs: device, n16, n32, flat16 (fp16 trainables), flat32 (fp32
    trainables) and after_weights_loaded().  `kernels` defaults to the HIP kernels; tests substitute host
    restatements to exercise the collective protocol on CPU ranks (gloo).  `weight` (finite, > 0) selects the
    sample-weighted layout and kernels (module docstring); None is the reference's plain mean.  `robust`
    ("median" | "trimmed_mean", with `trim_k` values cut at either end, or "multi_krum" with `krum_f` clients tolerated
    as wrong and `krum_m` kept, 0 = all but krum_f) selects the robust aggregation instead.
    `dp_clip` (finite, > 0) clips the client's update against the global copy to that L2 norm before it is packed, in
    whichever layout the bucket has (module docstring, DP-FedAvg).  `compress` ("int8" | "topk") sends the update
    compressed instead (module docstring), and `error_feedback` keeps what did not travel as a per-client residual
    (state_dict() / load_state_dict() carry it).  "int8": int8 codes with block scales, `compress_rounding` "nearest" |
    "stochastic", `compress_seed` and `client`, the global client index, selecting the stochastic rounding's bits.
    "topk": the `compress_k` (1..64) entries of largest magnitude of every block of 256 coordinates.  The bucket does not
    tell the two apart: its pack() asks its exchange to encode, which chose the codec when it was built.  `dyn` (the
    process's FedDynState) selects FedDyn (module docstring): the bucket keeps its client's correction `lam` and unpack()
    runs the round's end; not with weight, robust, dp_clip, compress or server.

    pack() / unpack() are the per-client halves; start() / finish() / run() exchange this one bucket
    alone (one client per rank: the bench and the single-client tests).  Several clients per rank
    exchange through one FedAvgExchange over all their buckets."""

    def __init__(self, engine, group: Optional[dist.ProcessGroup] = None, kernels=_HipKernels,
                 mode: str = "ordered", shard_single: bool = False, weight: Optional[float] = None,
                 server: Optional["ServerOptimizer"] = None, robust: Optional[str] = None, trim_k: int = 1,
                 dp_clip: Optional[float] = None, compress: Optional[str] = None, compress_rounding: str = "nearest",
                 error_feedback: bool = True, compress_seed: int = 0, client: int = 0,
                 dyn: Optional["FedDynState"] = None, compress_k: int = 8, krum_f: int = 1, krum_m: int = 0):
        if mode not in MODES:
            raise ValueError(f"FedAvg mode {mode!r}: one of {MODES}")
        if compress is not None and compress not in COMPRESS:
            raise ValueError(f"FedAvg compress {compress!r}: None or one of {COMPRESS}")
        if compress_rounding not in COMPRESS_ROUNDINGS:
            raise ValueError(f"FedAvg compress_rounding {compress_rounding!r}: one of {COMPRESS_ROUNDINGS}")
        if isinstance(compress_seed, bool) or not isinstance(compress_seed, int) or not 0 <= compress_seed < 2 ** 64:
            raise ValueError(f"FedAvg compress_seed {compress_seed!r}: an integer in [0, 2**64)")
        if isinstance(client, bool) or not isinstance(client, int) or not 0 <= client < 2 ** 31:
            raise ValueError(f"FedAvg client {client!r}: the global client index, an integer in [0, 2**31)")
        if isinstance(compress_k, bool) or not isinstance(compress_k, int) or not 1 <= compress_k <= TOPK_MAX:
            raise ValueError(f"FedAvg compress_k {compress_k!r}: an integer from 1 to {TOPK_MAX}")
        if compress is not None and dp_clip is not None:
            raise ValueError("FedAvg compress with dp_clip: a quantised, fed-back update no longer has an L2 norm "
                             "within the bound")
        if compress == "topk" and compress_rounding == "stochastic":
            raise ValueError('FedAvg compress "topk" with compress_rounding "stochastic": the kept values travel as '
                             "fp32, there is nothing to round")
        if compress == "topk" and robust is not None:
            raise ValueError('FedAvg compress "topk" with robust aggregation: most coordinates of every client decode '
                             "to the global copy itself, so a coordinate-wise median returns it unless half the "
                             "clients kept that coordinate")
        if dyn is not None:
            for label, on in (("a client weight", weight is not None), ("robust aggregation", robust is not None),
                              ("dp_clip", dp_clip is not None), ("compress", compress is not None),
                              ("a server optimizer", server is not None)):
                if on:
                    raise ValueError(f"FedAvg dyn with {label}: FedDyn's h is the mean of the clients' corrections "
                                     "only while the server sees the clients' own weights in a plain mean")
            if (dyn.n16, dyn.n32) != (engine.n16, engine.n32):
                raise ValueError("FedAvgBucket: the FedDyn state was built for other sizes")
        self.compress, self.compress_rounding, self.error_feedback = compress, compress_rounding, bool(error_feedback)
        self.compress_seed, self.client, self.compress_k = compress_seed, client, compress_k
        if dp_clip is not None:
            dp_clip = float(dp_clip)
            if not math.isfinite(dp_clip) or dp_clip <= 0.0:
                raise ValueError(f"FedAvg dp_clip {dp_clip}: finite and > 0 (None: no clipping)")
        self.dp_clip = dp_clip
        self.trim = robust_trim(robust, trim_k, mode, weight is not None)
        self.robust, self.trim_k = robust, trim_k
        self.krum_f, self.krum_m = check_krum(krum_f, krum_m) if robust == "multi_krum" else (krum_f, krum_m)
        if weight is not None:
            weight = float(weight)
            if not math.isfinite(weight) or weight <= 0.0:
                raise ValueError(f"FedAvg client weight {weight}: finite and > 0")
        self.weight = weight
        self.e = engine
        self.group = group
        self.k = kernels
        self.mode = mode
        self.shard_single = shard_single
        dev = engine.device
        n = engine.n16 + engine.n32
        self.world = _world(group)
        # [bucket | count | zero padding to a multiple of the world size]: one contiguous buffer so the
        # mean and the valid-client count travel in the same collectives.  With a client weight (every client
        # of a run has one or none): [weight * bucket | weight | count | padding], so the weighted sum, the sum
        # of the weights and the count travel together and the exchange itself is unchanged.  The robust
        # aggregation uses that layout at weight 1 ([bucket | 1 | count | padding])
        self.weighted = weight is not None or robust is not None
        tail = 2 if self.weighted else 1
        # compressed: a shard is a whole number of quantisation blocks
        quantum = self.world * (COMPRESS_BLOCK if compress is not None else 1)
        padded = -(-(n + tail) // quantum) * quantum
        self.pbuf = torch.zeros(padded, device=dev, dtype=torch.float32)
        self.buf = self.pbuf[:n + tail]
        self.bucket = self.buf[:n]
        self.count = self.buf[n + tail - 1:]
        self.flag = torch.zeros(1, device=dev, dtype=torch.int32)
        self.failed = False
        # DP-FedAvg: {norm, scale, clipped} of the client's update, written and read on the device, and the norm's
        # per-chunk partial sums
        self.clip_out = self.clip_ws = None
        if dp_clip is not None:
            self.clip_out = torch.tensor([0.0, 1.0, 0.0], device=dev, dtype=torch.float32)
            self.clip_ws = torch.zeros(kernels.dp_update_ws_floats(engine.n16, engine.n32), device=dev,
                                       dtype=torch.float32)
        # the last global weights (what broadcast_weights would load): restored when a round fails
        self.global16 = engine.flat16.detach().clone()
        self.global32 = engine.flat32.detach().clone()
        self._x: Optional[FedAvgExchange] = None
        # int8 compression of the uplink: the error-feedback residual e and the buffer the quantiser writes e' to
        # (unpack() swaps them once per round), and the exchange whose send image this bucket's pack() writes, with
        # the bucket's place in it
        self.resid = self.resid_next = None
        if compress is not None and self.error_feedback:
            self.resid = torch.zeros(n, device=dev, dtype=torch.float32)
            self.resid_next = torch.zeros(n, device=dev, dtype=torch.float32)
        self._resid_due = False
        self._wire: Optional[tuple] = None
        if server is not None and (server.n16, server.n32) != (engine.n16, engine.n32):
            raise ValueError("FedAvgBucket: the server optimizer was built for other sizes")
        self.server = server
        # FedDyn: this client's correction lam_k, updated in place by unpack() (the captured step holds its pointer)
        self.dyn = dyn
        self.lam = None if dyn is None else torch.zeros(n, device=dev, dtype=torch.float32)

    # -- per client
    def pack(self, failed: bool = False):
        """Validity scan + pack.  failed=True: the client's local training raised (its weights are
        excluded, trainers/maple_fed.py:262-265); an invalid client contributes zeros and no vote
        (:272-277).  With compress the pack is the exchange's encoder: it writes this client's chunks of the exchange's send
        image and the next residual, and the fp32 bucket is filled by the decode."""
        e = self.e
        self.failed = failed
        if failed:
            self.flag.fill_(1)
        else:
            self.flag.zero_()
            self.k.nonfinite_flag(e.flat16, self.flag)
            self.k.nonfinite_flag(e.flat32, self.flag)
        if self.compress is not None:
            # the update against the weights the round started from, in the exchange's codec straight into its send
            # image; e is read, e' written: a late-failure re-pack reads the same e, weights, global copy and round
            # and reproduces the chunks, and unpack() commits e' once
            if self._wire is None:
                self.exchange  # this bucket alone: its exchange owns the image
            x, slot = self._wire
            x.encode(self, slot)
            self._resid_due = self.resid is not None and not failed
        elif self.dp_clip is not None and not failed:
            # the update against the weights the round started from, its clip scale left on the device for the pack
            self.k.dp_update_scale(e.flat16, self.global16, e.flat32, self.global32, self.dp_clip, self.clip_ws,
                                   self.clip_out)
            layout = "robust" if self.robust is not None else ("plain" if self.weight is None else "weighted")
            self.k.fedavg_pack_clipped(e.flat16, e.flat32, self.global16, self.global32, self.flag,
                                       self.clip_out[1:2], self.weight, layout, self.buf)
        elif self.robust is not None:
            self.k.fedavg_pack_robust(e.flat16, e.flat32, self.flag, self.buf)
        elif self.weight is None:
            self.k.fedavg_pack(e.flat16, e.flat32, self.flag, self.buf)
        else:
            self.k.fedavg_pack_weighted(e.flat16, e.flat32, self.flag, self.weight, self.buf)
        if self.server is not None:
            self.server.pending = True  # a new exchange: its first unpack applies the server step
        if self.dyn is not None:
            self.dyn.pending = True  # ... steps h

    def unpack(self):
        """The fp16-rounded mean into every trainable (device-side n_valid; n_valid == 0 leaves the weights
        at the previous global copy).  No host synchronisation.  With a server optimizer: the first unpack after
        the rank's packs applies the server step to the summed bucket and writes this client; the other local
        clients receive the same fp16(x) (deliver), so the step runs once per exchange -- a late-failure
        re-exchange packs again before any unpack and changes nothing about that.  With dyn the same holds for FedDyn's
        round end: the first unpack steps h, the others deliver, each updates its own lam unless its flag is set."""
        e = self.e
        sv = self.server
        dyn = self.dyn
        if dyn is not None:
            if dyn.pending:
                self.k.feddyn_step(self.buf, dyn.alpha, dyn.num_clients, dyn.h, self.lam, self.flag, e.flat16,
                                   e.flat32, self.global16, self.global32)
                dyn.pending = False
            else:
                self.k.feddyn_deliver(self.buf, dyn.alpha, dyn.h, self.lam, self.flag, e.flat16, e.flat32,
                                      self.global16, self.global32)
        elif sv is not None:
            if sv.pending:
                self.k.fedopt_step(self.buf, self.weighted, sv.name, sv.beta1, sv.beta2, sv.tau, sv.lr,
                                   sv.x, sv.m, sv.v, e.flat16, e.flat32, self.global16, self.global32)
                sv.pending = False
            else:
                self.k.fedopt_deliver(sv.x, e.flat16, e.flat32, self.global16, self.global32)
        elif not self.weighted:
            self.k.fedavg_unpack(self.buf, e.flat16, e.flat32, self.global16, self.global32)
        else:
            self.k.fedavg_unpack_weighted(self.buf, e.flat16, e.flat32, self.global16, self.global32)
        if self._resid_due:  # the residual of the codes that were exchanged, once per round; a failed client keeps its own
            self.resid, self.resid_next = self.resid_next, self.resid
            self._resid_due = False
        e.after_weights_loaded()

    def snapshot(self):
        """Take the engine's current weights as the global copy (after a checkpoint load or an explicit
        broadcast_weights: what an all-failed round reverts to)."""
        self.global16.copy_(self.e.flat16)
        self.global32.copy_(self.e.flat32)
        if self.server is not None:
            self.server.reset_from(self)
        if self.dyn is not None:  # weights from outside the round loop: the corrections restart, h stays their mean
            self.lam.zero_()
            self.dyn.reset()

    def n_valid(self) -> int:
        """Valid clients of the last round (host sync)."""
        return int(round(float(self.count.item())))

    def clip_stats(self):
        """(norm, scale) of the update the last pack() clipped (host sync; for logging).  (nan, 1.0) without dp_clip
        or when that pack was of a failed client, whose update was not measured."""
        if self.dp_clip is None or self.failed:
            return float("nan"), 1.0
        norm, scale = self.clip_out[:2].tolist()
        return norm, scale

    def state_dict(self) -> dict:
        """The error-feedback residual as a CPU fp32 tensor (None without one) and, under FedDyn, the correction lam
        next to it; torch.load(..., weights_only=True) reads it."""
        sd = {"residual": None if self.resid is None else self.resid.detach().cpu().clone()}
        if self.lam is not None:
            sd["lam"] = self.lam.detach().cpu().clone()
        return sd

    def load_state_dict(self, sd: dict):
        """A saved residual and lam (an absent or None entry zeroes this bucket's).  ValueError when this bucket keeps
        none, or for another size or dtype."""
        lam = sd.get("lam")
        if lam is not None:
            if self.lam is None:
                raise ValueError("FedAvgBucket state: a lam for a bucket without FedDyn")
            if not isinstance(lam, torch.Tensor) or lam.dtype != torch.float32 or lam.numel() != self.lam.numel():
                raise ValueError(f"FedAvgBucket state: lam is not fp32 of {self.lam.numel()} elements")
        if self.lam is not None:
            if lam is None:
                self.lam.zero_()
            else:
                self.lam.copy_(lam.reshape(-1))
        t = sd.get("residual")
        if t is None:
            if self.resid is not None:
                self.resid.zero_()
            return
        if self.resid is None:
            raise ValueError("FedAvgBucket state: a residual for a bucket without error feedback")
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != self.resid.numel():
            raise ValueError(f"FedAvgBucket state: the residual is not fp32 of {self.resid.numel()} elements")
        self.resid.copy_(t.reshape(-1))
        self._resid_due = False

    # -- this bucket alone
    @property
    def exchange(self) -> "FedAvgExchange":
        if self._x is None:
            self._x = FedAvgExchange([self], group=self.group, mode=self.mode, shard_single=self.shard_single,
                                     robust=self.robust, trim_k=self.trim_k, krum_f=self.krum_f, krum_m=self.krum_m)
        return self._x

    @property
    def sharded(self) -> bool:
        return self.exchange.sharded

    @property
    def side(self):
        return self.exchange.side

    def start(self, collective: bool = True, failed: bool = False):
        """pack + (async) exchange; returns immediately (the caller overlaps the collective with test()).
        collective=False packs only."""
        self.pack(failed)
        if collective:
            self.exchange.start()
        elif self.compress is not None:  # packed only: the bucket still has to hold the fp32 image of its codes
            self._wire[0].decode_local()

    def finish(self, late_failed: Optional[bool] = None):
        """Wait for the exchange, then unpack.  late_failed: whether the client failed after start()
        (None: the caller ran nothing that can fail in between -- no agreement collective)."""
        if self._x is not None and self._x.started:
            self._x.finish(None if late_failed is None else ([0] if late_failed else []))
        self.unpack()

    def run(self) -> int:
        self.start()
        self.finish()
        return self.n_valid()


class FedAvgExchange:
    """The exchange of one rank's buckets (its C clients, in client order) with every other rank's.  With compress it
    owns the uint8 send image and the codec: the constructor picks, once, the chunk size and the encode and decode
    kernels of "int8" or "topk", and encode(), decode_local() and the sharded chain call what it picked."""

    def __init__(self, buckets: Sequence[FedAvgBucket], group: Optional[dist.ProcessGroup] = None,
                 mode: str = "ordered", shard_single: bool = False, robust: Optional[str] = None, trim_k: int = 1,
                 dp_std: float = 0.0, dp_seed: int = 0, krum_f: int = 1, krum_m: int = 0):
        if mode not in MODES:
            raise ValueError(f"FedAvg mode {mode!r}: one of {MODES}")
        dp_std = float(dp_std)
        if not math.isfinite(dp_std) or dp_std < 0.0:
            raise ValueError(f"FedAvg dp_std {dp_std}: finite and >= 0")
        if isinstance(dp_seed, bool) or not isinstance(dp_seed, int) or not 0 <= dp_seed < 2 ** 64:
            raise ValueError(f"FedAvg dp_seed {dp_seed!r}: an integer in [0, 2**64)")
        self.b = list(buckets)
        if len({None if x.compress is None else (x.compress, x.compress_rounding, x.error_feedback, x.compress_seed,
                                                 x.compress_k) for x in self.b}) > 1:
            raise ValueError("FedAvg compress: the buckets of one exchange differ in their compression settings")
        assert self.b and len({x.pbuf.numel() for x in self.b}) == 1
        # one layout per exchange: every bucket weighted (n + 2 floats) or none (n + 1)
        assert len({x.weight is None for x in self.b}) == 1, "weighted and unweighted buckets in one exchange"
        self.trim = robust_trim(robust, trim_k, mode, self.b[0].weight is not None)
        assert all(x.trim == self.trim for x in self.b), "the buckets and their exchange differ in robust / trim_k"
        self.krum = robust == "multi_krum"
        if self.krum:
            self.krum_f, self.krum_m = check_krum(krum_f, krum_m)
            assert all((x.krum_f, x.krum_m) == (krum_f, krum_m) for x in self.b), \
                "the buckets and their exchange differ in krum_f / krum_m"
        b0 = self.b[0]
        if dp_std > 0.0:
            if any(x.dp_clip is None for x in self.b):
                raise ValueError("FedAvg dp_std > 0 needs dp_clip on every bucket: unclipped updates have no sensitivity")
            if b0.weight is not None:
                raise ValueError("FedAvg dp_std > 0 with a client weight: the sensitivity would be w_k S / sum w")
            if self.trim is not None:
                raise ValueError("FedAvg dp_std > 0 with robust aggregation: an order statistic has a different "
                                 "sensitivity")
        # DP-FedAvg noise: N(0, dp_std^2) on each of the n summed coordinates, a function of (seed, round, coordinate)
        self.dp_std, self.dp_seed, self.round = dp_std, dp_seed, 0
        self.n = b0.bucket.numel()
        self._noise_due = False
        self.group, self.mode, self.k = group, mode, b0.k
        self.C = len(self.b)
        self.world = _world(group)
        self.distributed = dist.is_available() and dist.is_initialized() and (self.world > 1 or shard_single)
        dev = b0.pbuf.device
        padded = b0.pbuf.numel()
        self.S = padded // self.world
        # shard_single: run the sharded ordered exchange even in a one-rank group (tests drive the RCCL
        # all_to_all -> reduce -> all_gather chain on a one-GPU box this way)
        self.sharded = self.distributed and mode == "ordered"
        self.side = None
        self.host_stage = False
        # compression of the uplink: one setting per exchange; the uint8 send image [dest rank][client][chunk] the
        # buckets' packs write into, and under the sharded chain the image the all_to_all fills
        self.compress = b0.compress
        self.image = self.recv_image = self.topk = None
        if self.compress is not None:
            if b0.compress_rounding == "stochastic" and len({x.client for x in self.b}) != self.C:
                raise ValueError("FedAvg compress: two buckets of one exchange carry the same client index (their "
                                 "rounding bits would coincide)")
            self.layout = "robust" if b0.robust is not None else ("plain" if b0.weight is None else "weighted")
            # the one place that tells the codecs apart: the chunk size, the encode and decode kernels, and the
            # arguments each takes of its own (encode: after the weight, from the bucket; decode: last)
            kn = self.k
            if self.compress == "topk":
                self.topk = b0.compress_k
                self.chunk = kn.topk_chunk_bytes(self.S, self.topk)
                self._encode, self._encode_args = kn.topk_select, lambda x: (self.topk,)
                self._decode, self._decode_args = kn.topk_decode, (self.topk,)
            else:
                self.chunk = kn.compress_chunk_bytes(self.S)
                self._encode = kn.compress_quantize
                self._encode_args = lambda x: (x.compress_rounding, x.compress_seed, self.round, x.client)
                self._decode, self._decode_args = kn.compress_decode, ()
            self.image = torch.zeros(self.world, self.C, self.chunk, device=dev, dtype=torch.uint8)
            if self.sharded:
                self.recv_image = torch.empty(self.world * self.C * self.chunk, device=dev, dtype=torch.uint8)
            for j, x in enumerate(self.b):
                x._wire = (self, j)
        # the exchange's send image: C == 1 sends the bucket itself; C > 1 stages [dest rank][client][shard]
        self.stage = None if self.C == 1 or self.compress is not None else torch.empty(
            self.world, self.C, self.S, device=dev, dtype=torch.float32)
        # where the exchanged sum lands (C == 1: back into the bucket; C > 1: a total copied into every bucket)
        self.total = b0.pbuf if self.C == 1 else torch.empty(padded, device=dev, dtype=torch.float32)
        self.recv = self.shard = None
        if self.sharded:
            self.recv = torch.empty(self.world * self.C * self.S, device=dev, dtype=torch.float32)
            self.shard = torch.empty(self.S, device=dev, dtype=torch.float32)
        if self.distributed:
            # RCCL on GPUs: the chain on a side stream.  Other backends (gloo: the CPU tests, and the
            # several-ranks-on-one-GPU rehearsal of bench.py) exchange host copies in finish().
            self.host_stage = dev.type == "cuda" and dist.get_backend(group) != "nccl"
            if dev.type == "cuda" and not self.host_stage:
                self.side = torch.cuda.Stream(device=dev)
        # robust, one process: the rank's buckets staged [client][coordinate], the image the trimmed reduce reads
        self.local_stage = None
        if self.trim is not None and not self.distributed:
            self.local_stage = torch.empty(self.C, padded, device=dev, dtype=torch.float32)
        self.count_pos = b0.buf.numel() - 1  # the vote element, the last of the bucket
        # Multi-Krum: this rank's fp64 distance matrix over its coordinates, the W ranks' matrices gathered, the pairwise
        # kernel's workspace, and the selection every rank computes identically from the same W parts
        if self.krum:
            nc = self.world * self.C if self.sharded else self.C
            span = self.S if self.sharded else padded
            self.kn = nc
            self.kpart = torch.zeros(nc * nc, device=dev, dtype=torch.float64)
            self.kparts = torch.zeros(self.world * nc * nc, device=dev, dtype=torch.float64) if self.sharded else None
            self.kws = torch.zeros(-(-self.k.krum_ws_bytes(nc, span) // 8), device=dev, dtype=torch.float64)
            self.selected = torch.zeros(nc, device=dev, dtype=torch.int32)
            self.scores = torch.zeros(nc, device=dev, dtype=torch.float64)
            self.kcounts = torch.zeros(3, device=dev, dtype=torch.int32)
        self.started = False
        self.work = None

    def _send_image(self) -> torch.Tensor:
        if self.C == 1:
            return self.b[0].pbuf
        for j, x in enumerate(self.b):
            self.stage[:, j, :].copy_(x.pbuf.view(self.world, self.S))
        return self.stage.view(-1)

    def encode(self, x: FedAvgBucket, slot: int):
        """Bucket x's pack under compression: its update and the tail, in this exchange's codec, into its chunks
        image[:, slot, :] of the send image, and its next residual."""
        e = x.e
        self._encode(e.flat16, e.flat32, x.global16, x.global32, x.resid, x.resid_next, x.flag, x.weight,
                     *self._encode_args(x), self.image, slot, self.S)

    def decode_local(self):
        """Compressed, without the sharded chain (one process, "allreduce"): every local bucket's chunks decoded into
        its own fp32 bucket, g + what travelled in the bucket's layout, which the existing paths then consume.  No
        traffic is saved here: the compression is simulated."""
        img = self.image.view(-1)
        for j, x in enumerate(self.b):
            self._decode(img[j * self.chunk:], self.world, self.C * self.chunk, self.S, 0, self.S, x.global16,
                         x.global32, self.layout, x.pbuf, self.S, *self._decode_args)

    def _local_sum(self) -> torch.Tensor:
        """The rank's buckets summed in client order (== torch.stack(...) order over these clients)."""
        if self.C == 1:
            return self.b[0].pbuf
        self.total.copy_(self.b[0].pbuf)
        for x in self.b[1:]:
            self.total.add_(x.pbuf)
        return self.total

    def _local_robust(self) -> torch.Tensor:
        """The robust statistic over the rank's buckets (one process): the kernel of the sharded chain over the whole
        bucket.  It runs for a single client too: it turns an invalid client's absence marks into a zero vote."""
        for j, x in enumerate(self.b):
            self.local_stage[j].copy_(x.pbuf)
        if self.krum:  # one part: the distances over the whole bucket
            self.k.krum_pairwise(self.local_stage.view(-1), self.C, self.local_stage.shape[1], self.kws, self.kpart)
            self.k.krum_select(self.kpart, self.C, self.krum_f, self.krum_m, self.selected, self.scores, self.kcounts)
            self.k.fedavg_reduce_selected(self.local_stage.view(-1), self.C, self.selected, self.count_pos, self.total)
            return self.total
        self.k.fedavg_reduce_trimmed(self.local_stage.view(-1), self.C, self.trim, self.count_pos, self.total)
        return self.total

    def start(self):
        """Launch the exchange of the packed buckets (asynchronously where the backend allows)."""
        self.started = True
        self.work = None
        self._noise_due = self.dp_std > 0.0 and not self.sharded  # the sharded chain noises its shard itself
        if not self.distributed:
            return  # one process: the sum is formed in finish()
        if not self.sharded:
            if self.compress is not None:
                self.decode_local()
            src = self._local_sum()
            if src is not self.total:
                self.total.copy_(src)
            self.work = dist.all_reduce(self.total, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            return
        send = self._send_image() if self.compress is None else self.image.view(-1)  # the packs wrote it in place
        if self.side is not None:
            # the whole chain on the side stream: the current stream only waits for it in finish()
            self.side.wait_stream(torch.cuda.current_stream(send.device))
            with torch.cuda.stream(self.side):
                self.work = self._ordered_chain(send)
        else:  # gloo: the same chain, its waits host waits
            self.work = self._ordered_chain(send)

    def _ordered_chain(self, send: torch.Tensor):
        """all_to_all of the shards -> client-ordered sum (robust: the trimmed reduce) of this rank's shard ->
        all_gather of the results.
        One code path for every backend: under RCCL (on the side stream) a2a.wait() is a stream dependency;
        under gloo it is a host wait, and with device buckets (host_stage) the collectives move host copies.
        Returns the all_gather's work handle (None when it completed here)."""
        hs = self.host_stage
        into = self.recv if self.compress is None else self.recv_image  # the fp32 image, or the uint8 one
        recv = torch.empty(into.numel(), dtype=into.dtype) if hs else into
        a2a = dist.all_to_all_single(recv, send.cpu() if hs else send, group=self.group, async_op=True)
        a2a.wait()
        if hs:
            into.copy_(recv)
        if self.compress is not None:
            # the uint8 image moved; the receiver rebuilds the fp32 image g + what travelled of its shard of every
            # client from the global copy every rank holds, and the rest of the chain reads it as a received one
            b0 = self.b[0]
            self._decode(self.recv_image, self.world * self.C, self.chunk, self.S, dist.get_rank(self.group) * self.S,
                         0, b0.global16, b0.global32, self.layout, self.recv, self.S, *self._decode_args)
        if self.trim is None:
            self.k.fedavg_reduce_ordered(self.recv, self.world * self.C, self.shard)
        elif self.krum:
            # the distances over this rank's coordinates, every rank's part to every rank (W * N^2 doubles), the same
            # selection on every rank from the same parts in the same order, then the mean of the kept clients
            pos = self.count_pos - dist.get_rank(self.group) * self.S
            self.k.krum_pairwise(self.recv, self.kn, self.S, self.kws, self.kpart)
            if hs:
                parts = torch.empty(self.kparts.numel(), dtype=torch.float64)
                dist.all_gather_into_tensor(parts, self.kpart.cpu(), group=self.group)
                self.kparts.copy_(parts)
            else:
                dist.all_gather_into_tensor(self.kparts, self.kpart, group=self.group, async_op=True).wait()
            self.k.krum_select(self.kparts, self.kn, self.krum_f, self.krum_m, self.selected, self.scores, self.kcounts)
            self.k.fedavg_reduce_selected(self.recv, self.kn, self.selected, pos if 0 <= pos < self.S else -1,
                                          self.shard)
        else:  # the robust statistic of this rank's shard; the vote element, if it lies in this shard, counts
            pos = self.count_pos - dist.get_rank(self.group) * self.S
            self.k.fedavg_reduce_trimmed(self.recv, self.world * self.C, self.trim, pos if 0 <= pos < self.S else -1,
                                         self.shard)
        if self.dp_std > 0.0:  # this rank's part of the summed coordinates [0, n): global offset rank * S
            first = dist.get_rank(self.group) * self.S
            n_noise = min(max(self.n - first, 0), self.S)
            if n_noise > 0:
                self.k.dp_add_noise(self.shard[:n_noise], first, self.dp_seed, self.round, self.dp_std)
        if hs:
            out = torch.empty(self.total.numel(), dtype=torch.float32)
            dist.all_gather_into_tensor(out, self.shard.cpu(), group=self.group)
            self.total.copy_(out)
            return None
        return dist.all_gather_into_tensor(self.total, self.shard, group=self.group, async_op=True)

    def _complete(self):
        if self.work is not None:
            self.work.wait()
            self.work = None
        if not self.distributed:
            if self.compress is not None:
                self.decode_local()
            if self.trim is None:
                self._local_sum()
            else:
                self._local_robust()
        if self._noise_due:  # "allreduce" and one process: the whole sum, the same bits on every rank
            self._noise_due = False
            self.k.dp_add_noise(self.total[:self.n], 0, self.dp_seed, self.round, self.dp_std)
        if self.total is not self.b[0].pbuf:
            for x in self.b:
                x.pbuf.copy_(self.total)

    def _agree(self, code: int) -> int:
        """Max over the ranks of a small status code (0 ok, 1 a late client failure, 2 a rank aborts)."""
        if not self.distributed:
            return code
        dev = self.b[0].pbuf.device
        on_dev = dev.type == "cuda" and not self.host_stage
        t = torch.tensor([code], dtype=torch.int32, device=dev if on_dev else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return int(t.item())

    def finish(self, late_failed: Optional[Iterable[int]] = (), abort: bool = False):
        """Wait for the exchange; afterwards every local bucket holds the sum over all clients (unpack
        follows).  late_failed: local client indices that failed after they were packed (None: nothing ran
        between start and finish that can fail, so the ranks skip agreeing on it).  abort: this rank hit an
        error the reference does not catch (e.g. the ValueError of a non-finite input, trainers/maple.py:
        526-535); every rank then raises FederatedAbort instead of waiting in the next round's collectives."""
        late = sorted(set(late_failed)) if late_failed is not None else None
        code = self._agree(2 if abort else int(bool(late))) if late is not None else 0
        if code == 2:
            self._complete()
            self.started = False
            raise FederatedAbort("a rank stopped the federated run (an error the round loop does not catch)")
        if code == 1:
            self._complete()  # drain the exchange in flight (every rank does, in the same order)
            for j, x in enumerate(self.b):
                x.pack(failed=x.failed or j in late)
            self.start()
        self._complete()
        self.started = False
        self.round += 1  # once per finished round: the late-failure re-exchange above used the same value

    def state_dict(self) -> dict:
        """The noise stream's position: plain numbers (torch.load(..., weights_only=True) reads it)."""
        return {"round": self.round, "seed": self.dp_seed}

    def load_state_dict(self, sd: dict):
        """Continue a saved run's noise stream: its seed, and its round counter, so no (seed, round) pair recurs."""
        rnd, seed = sd.get("round"), sd.get("seed")
        for label, v, top in (("round", rnd, 2 ** 32), ("seed", seed, 2 ** 64)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < top:
                raise ValueError(f"FedAvgExchange state: {label} {v!r} is not an integer in [0, {top})")
        self.round, self.dp_seed = rnd, seed

    def n_valid(self) -> int:
        return self.b[0].n_valid()

    def krum_stats(self):
        """Multi-Krum's last selection (one host sync; for logging): (the kept clients' global ids, ascending -- the
        image's row order is the global client order --, every client's score with NaN for an absent one, p present,
        the effective f', the number kept m')."""
        if not self.krum:
            raise ValueError('krum_stats: the exchange was not built with robust="multi_krum"')
        flat = torch.cat([self.selected.double(), self.kcounts.double(), self.scores]).cpu()
        nc = self.kn
        kept = [c for c in range(nc) if flat[c] != 0]
        p, fe, me = (int(v) for v in flat[nc:nc + 3])
        return kept, flat[nc + 3:].tolist(), p, fe, me
