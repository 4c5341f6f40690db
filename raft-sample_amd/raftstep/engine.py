"""Python handle over libraftstep.so (the HIP engine), through the C-ABI only.

There is deliberately no CPU fallback: if the library or a GPU is missing
the constructor raises. The CPU restatement lives in oracle/ and is test
infrastructure, never imported from here.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RAFTSTEP_LIB") or os.path.normpath(os.path.join(_HERE, "..", "lib", "libraftstep.so"))   # env: A/B of another build
_lib = None


class RaftError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"raftstep error {code}: {msg}")
        self.code = code


def load_library(path=None):
    """Load and bind libraftstep.so; raises if it is missing (no fallback)."""
    global _lib
    if _lib is None or path:
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise RaftError(-2, f"{p} not built (run __graft_entry__.build() or make -C raft-sample_amd/csrc)")
        _lib = abi.bind(C.CDLL(p))
    return _lib


def _check(rc):
    if rc != 0:
        raise RaftError(rc, load_library().raft_last_error().decode(errors="replace"))


def stream_probe(device=0, replicas=5, elems=1 << 24, reps=10, heartbeat=True, flags=0):
    """The steady lean kernel's byte mix on fresh buffers (raft_stream_probe):
    (us per pass, bytes per pass). heartbeat=False: without the heartbeat
    store (a group in shared form; abi.PROBE_NO_HEARTBEAT). `flags`: further
    abi.PROBE_* bits (store policies, A/B)."""
    lib = load_library()
    us, by = C.c_double(), C.c_double()
    f = int(flags) | (0 if heartbeat else abi.PROBE_NO_HEARTBEAT)
    _check(lib.raft_stream_probe(int(device), int(replicas), int(elems), int(reps), f, C.byref(us), C.byref(by)))
    return us.value, by.value


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


class Engine:
    """One engine = the groups of one GPU (config.group_base.. +groups)."""

    def __init__(self, cfg=None, **kw):
        self.lib = load_library()
        self.cfg = cfg if cfg is not None else abi.default_config(**kw)
        if cfg is not None and kw:
            for k, v in kw.items():
                setattr(self.cfg, k, v)
        h = C.c_void_p()
        _check(self.lib.raft_engine_create(C.byref(self.cfg), C.byref(h)))
        self.h = h

    # -- lifecycle -----------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.raft_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def groups(self):
        return self.cfg.groups

    @property
    def replicas(self):
        return self.cfg.replicas

    def device_bytes(self):
        b = C.c_uint64()
        _check(self.lib.raft_engine_info(self.h, None, C.byref(b)))
        return b.value

    def features(self):
        """Storage forms in use (raft_engine_features): shared_entries,
        virtual_suffixes. Results are identical either way."""
        f = C.c_uint32()
        if hasattr(self.lib, "raft_engine_features"):
            _check(self.lib.raft_engine_features(self.h, C.byref(f)))
        return {"shared_entries": bool(f.value & abi.FEATURE_SHARED_ENTRIES),
                "virtual_suffixes": bool(f.value & abi.FEATURE_VIRTUAL_SUFFIXES)}

    # -- state ---------------------------------------------------------
    def init_new_nodes(self, tick0=0):
        _check(self.lib.raft_init_new_nodes(self.h, tick0))

    def init_steady(self, leader=0, tick0=0):
        _check(self.lib.raft_init_steady(self.h, leader, tick0))

    def store_state(self, logs=True):
        st = abi.empty_state(self.cfg.groups, self.cfg.replicas, self.cfg.ring_depth)
        if not logs:
            for k in ("log_term", "log_value", "log_crc"):
                st.pop(k)
        v = abi.make_view(st)
        _check(self.lib.raft_store_state(self.h, C.byref(v)))
        return st

    def store_state_range(self, first_group, n_groups, logs=True):
        """Canonical view of groups [first_group, first_group + n_groups) only (local indices)."""
        st = abi.empty_state(n_groups, self.cfg.replicas, self.cfg.ring_depth)
        if not logs:
            for k in ("log_term", "log_value", "log_crc"):
                st.pop(k)
        v = abi.make_view(st)
        _check(self.lib.raft_store_state_range(self.h, first_group, n_groups, C.byref(v)))
        return st

    def load_state(self, st):
        st = abi.coerce_state(st, self.cfg.groups, self.cfg.replicas, self.cfg.ring_depth)
        v = abi.make_view(st)
        _check(self.lib.raft_load_state(self.h, C.byref(v)))

    # -- audit ---------------------------------------------------------
    def state_digest(self):
        """(per-group digests u64[G], wrapping sum), computed on the device."""
        per = np.zeros(self.cfg.groups, np.uint64)
        tot = C.c_uint64()
        _check(self.lib.raft_state_digest(self.h, _ptr(per), C.byref(tot)))
        return per, tot.value

    def nodelog(self, group):
        """main.go nodelog lines (main.go:399-401) of every replica of `group`."""
        buf = C.create_string_buffer(64 * (self.cfg.replicas + 1))
        n = self.lib.raft_nodelog(self.h, group, buf, len(buf))
        if n < 0:
            _check(n)
        return buf.value.decode()

    def save_checkpoint(self, path):
        _check(self.lib.raft_checkpoint_save(self.h, os.fsencode(path)))

    def load_checkpoint(self, path):
        _check(self.lib.raft_checkpoint_load(self.h, os.fsencode(path)))

    # -- commit feed ---------------------------------------------------
    def feed_open(self, replicas=None, start="commit", cursors=None):
        """Open the commit feed (raft_feed_open). replicas: an iterable of
        replica ids or a bit mask, None = all. start: "start" (cursors 0),
        "commit" (only what commits from now on) or "cursors" (the [G][R]
        int32 array given, e.g. what feed_cursors() returned)."""
        R = self.cfg.replicas
        if replicas is None:
            mask = (1 << R) - 1
        elif isinstance(replicas, (int, np.integer)):
            mask = int(replicas)
        else:
            mask = 0
            for r in replicas:
                if int(r) < 0:
                    raise ValueError(f"replica {r}")
                mask |= 1 << int(r)
        if not 0 <= mask < 1 << 32:
            raise ValueError(f"replica mask {mask:#x}")
        cur = None
        if cursors is not None:
            cur = np.ascontiguousarray(cursors, dtype=np.int32)
            if cur.shape != (self.cfg.groups, R):
                raise ValueError(f"feed cursors: shape {cur.shape}, expected ({self.cfg.groups}, {R})")
        st = abi.FEED_START[start] if isinstance(start, str) else int(start)
        _check(self.lib.raft_feed_open(self.h, mask, st, _ptr(cur)))

    def feed_poll(self, cap=None):
        """Drain newly committed entries (raft_feed_poll): (FEED_ENTRY array
        ordered by (group, replica, index), info dict with delivered, pending,
        lost, stalled). cap=None counts first, then takes everything."""
        info = abi.FeedInfo()
        first = None
        if cap is None:
            _check(self.lib.raft_feed_poll(self.h, None, 0, C.byref(info)))
            first = info.lost, info.stalled   # (the counting poll already skipped the lost entries)
            cap = info.pending
        out = np.zeros(int(cap), abi.FEED_ENTRY)
        _check(self.lib.raft_feed_poll(self.h, _ptr(out), int(cap), C.byref(info)))
        d = {k: int(getattr(info, k)) for k, _ in abi.FeedInfo._fields_}
        if first is not None:
            d["lost"] += int(first[0])
            d["stalled"] = int(first[1])
        return out[:d["delivered"]], d

    def feed_cursors(self):
        """The feed's cursors, int32 [G][R]; -1 for replicas outside the mask."""
        out = np.zeros((self.cfg.groups, self.cfg.replicas), np.int32)
        _check(self.lib.raft_feed_cursors(self.h, _ptr(out)))
        return out

    def feed_close(self):
        _check(self.lib.raft_feed_close(self.h))

    # -- group directory -----------------------------------------------
    def group_scan(self, select, first_group=0, cap=None):
        """Groups in [first_group, G) that are faulted and / or leaderless
        (raft_group_scan; select: abi.SELECT_* bits): (GROUP_HIT array in
        ascending group order, info dict with matched, written, next_group).
        cap=None counts first, then takes every hit."""
        info = abi.ScanInfo()
        if cap is None:
            _check(self.lib.raft_group_scan(self.h, int(select), int(first_group), None, 0, C.byref(info)))
            cap = info.matched
        out = np.zeros(int(cap), abi.GROUP_HIT)
        _check(self.lib.raft_group_scan(self.h, int(select), int(first_group), _ptr(out), int(cap), C.byref(info)))
        d = {k: int(getattr(info, k)) for k, _ in abi.ScanInfo._fields_}
        return out[:d["written"]], d

    @staticmethod
    def _ids(ids):
        a = np.asarray(ids)
        if a.ndim != 1 or (a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0)):
            raise ValueError("group ids: a 1-D array of non-negative integers expected")
        return np.ascontiguousarray(a, dtype=np.uint64)

    def store_groups(self, ids, logs=True):
        """Canonical view of the listed groups (local ids, any order, repeats
        allowed), indexed by list position (raft_store_groups)."""
        ids = self._ids(ids)
        st = abi.empty_state(len(ids), self.cfg.replicas, self.cfg.ring_depth)
        if not logs:
            for k in ("log_term", "log_value", "log_crc"):
                st.pop(k)
        v = abi.make_view(st)
        _check(self.lib.raft_store_groups(self.h, _ptr(ids), len(ids), C.byref(v)))
        return st

    def restart_groups(self, ids, tick0):
        """NewNode x R for the listed (distinct) groups at virtual tick tick0 (raft_restart_groups)."""
        ids = self._ids(ids)
        _check(self.lib.raft_restart_groups(self.h, _ptr(ids), len(ids), int(tick0)))

    def load_groups(self, ids, rows):
        """Load the canonical view `rows` (what store_groups(ids) returns:
        indexed by list position, optional fields may be absent) into the
        listed (distinct) groups (raft_load_groups)."""
        ids = self._ids(ids)
        rows = abi.coerce_state(rows, len(ids), self.cfg.replicas, self.cfg.ring_depth)
        v = abi.make_view(rows)
        _check(self.lib.raft_load_groups(self.h, _ptr(ids), len(ids), C.byref(v)))

    # -- group audit ---------------------------------------------------
    def group_audit(self, checks=abi.AUDIT_ALL, first_group=0, cap=None):
        """Groups in [first_group, G) that violate one of the safety
        invariants `checks` names (raft_group_audit; abi.AUDIT_* bits):
        (AUDIT_HIT array in ascending group order, each with the witness of
        its lowest violated check; info dict with matched, written, next_group
        and per_check, the groups violating each check by abi.AUDIT_NAMES).
        cap=None counts first, then takes every hit."""
        info = abi.AuditInfo()
        if cap is None:
            _check(self.lib.raft_group_audit(self.h, int(checks), int(first_group), None, 0, C.byref(info)))
            cap = info.matched
        out = np.zeros(int(cap), abi.AUDIT_HIT)
        _check(self.lib.raft_group_audit(self.h, int(checks), int(first_group), _ptr(out), int(cap), C.byref(info)))
        d = dict(matched=int(info.matched), written=int(info.written), next_group=int(info.next_group),
                 per_check={k: int(info.per_check[i]) for i, k in enumerate(abi.AUDIT_NAMES)})
        return out[:d["written"]], d

    # -- client proposals ----------------------------------------------
    def propose(self, now_tick, groups, values):
        """Append values[i] to the log of every Leader of groups[i] (local ids,
        any order, repeats allowed; applied in list order) at virtual tick
        now_tick (raft_propose): the TICKET array, one per proposal."""
        ids = self._ids(groups)
        vals = np.asarray(values)
        if vals.shape != ids.shape or (vals.size and vals.dtype.kind not in "iu"):
            raise ValueError("proposal values: one integer per group id expected")
        props = np.zeros(len(ids), abi.PROPOSAL)
        props["group"] = ids
        props["value"] = vals.astype(np.int64)
        out = np.zeros(len(ids), abi.TICKET)
        _check(self.lib.raft_propose(self.h, int(now_tick), _ptr(props), len(props), _ptr(out)))
        return out

    def ticket_status(self, tickets, results=True):
        """What became of each ticket (raft_ticket_status; read-only):
        (TICKET_RESULT array, or None with results=False, which only counts;
        {state name: tickets} by abi.TICKET_STATE_NAMES)."""
        tickets = np.ascontiguousarray(tickets, dtype=abi.TICKET)
        info = abi.TicketInfo()
        out = np.zeros(len(tickets), abi.TICKET_RESULT) if results else None
        _check(self.lib.raft_ticket_status(self.h, _ptr(tickets), len(tickets), _ptr(out), C.byref(info)))
        return out, {k: int(info.per_state[i]) for i, k in enumerate(abi.TICKET_STATE_NAMES)}

    # -- applied state -------------------------------------------------
    def _replica_mask(self, replicas):
        R = self.cfg.replicas
        if replicas is None:
            return (1 << R) - 1
        if isinstance(replicas, (int, np.integer)):
            mask = int(replicas)
        else:
            mask = 0
            for r in replicas:
                if int(r) < 0:
                    raise ValueError(f"replica {r}")
                mask |= 1 << int(r)
        if not 0 <= mask < 1 << 32:
            raise ValueError(f"replica mask {mask:#x}")
        return mask

    def apply_open(self, replicas=None, start="commit", records=None):
        """Open the applied state (raft_apply_open). replicas: an iterable of
        replica ids or a bit mask, None = all. start: "start" (from index 0),
        "commit" (only what commits from now on) or "records" (the [G][R]
        APPLY_RECORD array given, e.g. what apply_read() returned)."""
        rec = None
        if records is not None:
            rec = np.ascontiguousarray(records, dtype=abi.APPLY_RECORD)
            if rec.shape != (self.cfg.groups, self.cfg.replicas):
                raise ValueError(f"apply records: shape {rec.shape}, expected ({self.cfg.groups}, {self.cfg.replicas})")
        st = abi.APPLY_START[start] if isinstance(start, str) else int(start)
        _check(self.lib.raft_apply_open(self.h, self._replica_mask(replicas), st, _ptr(rec)))

    def apply_step(self):
        """Fold what has committed since the last step into the records and
        compare the replicas of every group (raft_apply_step): a dict with
        folded, lost, stalled, gapped, diverged."""
        info = abi.ApplyInfo()
        _check(self.lib.raft_apply_step(self.h, C.byref(info)))
        return {k: int(getattr(info, k)) for k in abi.APPLY_INFO_NAMES}

    def apply_read(self, ids=None):
        """The records of the listed groups (local ids, any order, repeats
        allowed; None: all groups) as an APPLY_RECORD array [n][R]; replicas
        outside the mask read applied = -1 (raft_apply_read)."""
        R = self.cfg.replicas
        if ids is None:
            out = np.zeros((self.cfg.groups, R), abi.APPLY_RECORD)
            _check(self.lib.raft_apply_read(self.h, None, self.cfg.groups, _ptr(out)))
            return out
        ids = self._ids(ids)
        out = np.zeros((len(ids), R), abi.APPLY_RECORD)
        if len(ids):
            _check(self.lib.raft_apply_read(self.h, _ptr(ids), len(ids), _ptr(out)))
        return out

    def apply_scan(self, select, first_group=0, cap=None):
        """Groups in [first_group, G) with a diverged and / or a gapped
        replica (raft_apply_scan; select: abi.APPLY_DIVERGED | APPLY_GAPPED):
        (APPLY_HIT array in ascending group order, info dict with matched,
        written, next_group). cap=None counts first, then takes every hit."""
        info = abi.ScanInfo()
        if cap is None:
            _check(self.lib.raft_apply_scan(self.h, int(select), int(first_group), None, 0, C.byref(info)))
            cap = info.matched
        out = np.zeros(int(cap), abi.APPLY_HIT)
        _check(self.lib.raft_apply_scan(self.h, int(select), int(first_group), _ptr(out), int(cap), C.byref(info)))
        d = {k: int(getattr(info, k)) for k, _ in abi.ScanInfo._fields_}
        return out[:d["written"]], d

    def apply_close(self):
        _check(self.lib.raft_apply_close(self.h))

    # -- the fused tick ------------------------------------------------
    def tick(self, first_tick, nticks=1, stats=True):
        if stats:
            s = abi.TickStats()
            _check(self.lib.raft_tick(self.h, first_tick, nticks, C.byref(s)))
            return np.array(s.v, dtype=np.int64)
        _check(self.lib.raft_tick(self.h, first_tick, nticks, None))
        return None

    def stage_values(self, first_tick, values):
        """RAFT_CLIENT_STAGED: copy the client values of ticks first_tick ..
        first_tick + len(values) - 1 into HBM; values[t][e][g] int64
        (raft_stage_values: [nticks][E][G])."""
        v = np.ascontiguousarray(values, dtype=np.int64)
        if v.ndim != 3 or v.shape[1:] != (self.cfg.entries_per_tick, self.cfg.groups):
            raise ValueError(f"staged values: shape {v.shape}, expected (nticks, {self.cfg.entries_per_tick}, "
                             f"{self.cfg.groups})")
        _check(self.lib.raft_stage_values(self.h, int(first_tick), v.shape[0], _ptr(v)))

    def tick_records(self, nticks):
        """Per-tick stats [nticks][8] of the last tick(stats=True) call (device-reduced,
        summed over GPUs with a communicator)."""
        recs = (abi.TickStats * nticks)()
        _check(self.lib.raft_tick_records(self.h, nticks, recs))
        return np.array([list(r.v) for r in recs], dtype=np.int64).reshape(nticks, abi.NSTATS)

    def sync(self):
        _check(self.lib.raft_sync(self.h))

    # -- handler batches -----------------------------------------------
    def append_entries(self, now_tick, reqs, entries=None):
        reqs = np.ascontiguousarray(reqs, dtype=abi.AE_REQ)
        ents = np.ascontiguousarray(entries if entries is not None else np.zeros(0, abi.LOG_ENTRY),
                                    dtype=abi.LOG_ENTRY)
        out = np.zeros(len(reqs), abi.AE_RESP)
        _check(self.lib.raft_append_entries_batch(self.h, now_tick, _ptr(reqs), len(reqs), _ptr(ents),
                                                  len(ents), _ptr(out)))
        return out

    def request_vote(self, now_tick, reqs):
        reqs = np.ascontiguousarray(reqs, dtype=abi.VOTE_REQ)
        out = np.zeros(len(reqs), abi.VOTE_RESP)
        _check(self.lib.raft_request_vote_batch(self.h, now_tick, _ptr(reqs), len(reqs), _ptr(out)))
        return out

    def group_ops(self, now_tick, ops):
        ops = np.ascontiguousarray(ops, dtype=abi.GROUP_OP)
        out = np.zeros(len(ops), abi.OP_RESULT)
        _check(self.lib.raft_group_ops_batch(self.h, now_tick, _ptr(ops), len(ops), _ptr(out)))
        return out

    # -- multi-GPU -----------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        _check(load_library().raft_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        _check(self.lib.raft_comm_init(self.h, nranks, rank, buf))

    def comm_info(self):
        """(nranks, rank, allreduces issued) as RCCL reports them (1, 0, n without a communicator)."""
        n, r, k = C.c_int32(), C.c_int32(), C.c_uint64()
        _check(self.lib.raft_comm_info(self.h, C.byref(n), C.byref(r), C.byref(k)))
        return n.value, r.value, k.value

    def allreduce_stats(self, stats):
        s = abi.TickStats()
        for i, x in enumerate(stats):
            s.v[i] = int(x)
        _check(self.lib.raft_comm_allreduce_stats(self.h, C.byref(s)))
        return np.array(s.v, dtype=np.int64)

    # -- instrumentation -----------------------------------------------
    def profile(self, mode=1):
        """0 off, 1 per-dispatch events on the steady-state kernel, 2 one event pair per tick()
        call, 3 per-dispatch events on the two-pass plan's list kernel."""
        _check(self.lib.raft_profile_enable(self.h, int(mode)))

    def profile_read(self):
        ms, n = C.c_double(), C.c_uint64()
        _check(self.lib.raft_profile_read(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # -- diagnostics ---------------------------------------------------
    def diag_enable(self, on=True):
        """Zero and start (or stop) the tick-class counters (raft_diag_enable)."""
        _check(self.lib.raft_diag_enable(self.h, int(bool(on))))

    def diag_read(self):
        """{class name: lanes} since the last read (abi.DIAG names; raft_diag_read), then zeroed."""
        buf = (C.c_uint64 * abi.DIAG_COUNTERS)()
        _check(self.lib.raft_diag_read(self.h, buf, abi.DIAG_COUNTERS))
        return {k: int(buf[i]) for k, i in abi.DIAG.items()}

    def debug_group_words(self, group):
        """Raw per-group words (gmeta, giso, hb, gss[4], glx[2], grot, grota, gsb, grotb, gsb2)."""
        buf = (C.c_int32 * 14)()
        _check(self.lib.raft_debug_group_words(self.h, int(group), buf, 14))
        names = ("meta", "giso", "hb", "ss_last", "ss_term", "ss_cl", "ss_cf", "lx_k", "lx_dl", "rot", "rota", "sb",
                 "rotb", "sb2")
        return dict(zip(names, list(buf)))

    def debug_diag_mode(self, mode):
        """Timing diagnostics (results wrong while non-zero; engine created with
        debug_flags=abi.DEBUG_ALLOW_WRONG_RESULTS)."""
        _check(self.lib.raft_debug_diag_mode(self.h, int(mode)))

    def debug_force_pass(self, group):
        """Test knob: the lean kernel passes `group` (-1: none) to the list kernel."""
        _check(self.lib.raft_debug_force_pass(self.h, int(group)))
