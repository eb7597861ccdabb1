"""Python binding of librmc.so (include/rmc.h) — used by tests and bench.py.

The product is the HIP library; this module is a thin ctypes layer with the
same names and meanings as the C ABI.  It never falls back to a CPU path:
if `lib/librmc.so` is missing, importing `rmc.native()` raises.

TLC correspondence: `Config` = the .cfg bounds,
`Checker.run()` = `tlc2.TLC` BFS to fixpoint, `Result` = TLC's summary
("N states generated, M distinct states found, Q left on queue", depth).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "librmc.so")
if os.environ.get("RMC_LIB"):  # another in-tree build of librmc (same-box A/B of two builds)
    LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", os.environ["RMC_LIB"])

MAX_SERVERS, MAX_LOG, MAX_MSGS = 5, 3, 8  # the packed layout's capacity
WIDE_MAX_TERM, WIDE_MAX_LOG, WIDE_MAX_MSGS, WIDE_MAX_DUP = 255, 32, 64, 255  # the wide layout's
VIEW_LOG, VIEW_MSGS = 32, 64  # rmc_state_view sizes (RMC_VIEW_LOG, RMC_VIEW_MSGS)
SIM_WITHIN_CAPACITY, SIM_TRUNCATE, SIM_TLC = 0, 1, 2
FLAG_SYMMETRY, FLAG_CHECK_DEADLOCK, FLAG_BUG_QUORUM, FLAG_VERIFY_STATES, FLAG_SPILL = 1, 2, 4, 8, 16
INV_TYPEOK, INV_ONE_LEADER, INV_LOG_MATCHING, INV_MESSAGES = 1, 2, 4, 8
INV_LEADER_VOTES, INV_CAND_TERM = 16, 32
INV_VOTES_GRANTED, INV_QUORUM_LOG, INV_MORE_UP_TO_DATE, INV_LEADER_COMPLETE = 64, 128, 256, 512
INV_NAMES = {INV_TYPEOK: "TypeOK", INV_ONE_LEADER: "OneLeaderPerTerm",
             INV_LOG_MATCHING: "LogMatching", INV_MESSAGES: "MessagesInv",
             INV_LEADER_VOTES: "LeaderVotesQuorum", INV_CAND_TERM: "CandidateTermNotInLog",
             INV_VOTES_GRANTED: "VotesGrantedInv", INV_QUORUM_LOG: "QuorumLogInv",
             INV_MORE_UP_TO_DATE: "MoreUpToDateCorrect", INV_LEADER_COMPLETE: "LeaderCompleteness"}
FRONT_BUILTIN_RAFT, FRONT_SIMULATE, FRONT_DEPTH_BOUNDED, FRONT_PREDICATES = 1, 2, 4, 8
FRONT_CONSTRAINTS = 16   # RMC_FRONT_CONSTRAINTS: CONSTRAINT conjuncts that are no bound become residuals
FRONT_ACTIONS = 32       # RMC_FRONT_ACTIONS: a PROPERTY [][A]_vars is an action property
ACT_USER0 = 1 << 24      # RMC_ACT_USER0: action property p is bit 24 + p of Result.violated_inv
MAX_ACTION_PROPS = 4
MAX_PREDICATES = 8       # RMC_MAX_PREDICATES: model-defined invariants per program
INV_USER0 = 1 << 16      # RMC_INV_USER0: predicate p is bit 16 + p of Result.violated_inv
PRED_HOLDS, PRED_VIOLATED, PRED_ERROR = 0, 1, 2  # verdicts of rmc_eval_predicates
FLAG_UNBOUNDED_TERM, FLAG_UNBOUNDED_LOG, FLAG_UNBOUNDED_MSGS, FLAG_UNBOUNDED_DUP = 32, 64, 128, 256
FLAG_COVERAGE = 512
FLAG_CONTINUE = 2048  # (bit 10 is not assigned)
INV_COUNT = 10  # RMC_INV_COUNT: the rows of rmc_violations, bit r = 1 << r
# rows of rmc_coverage (RMC_COV_ACTIONS; rmc_coverage_action): Init, the server families, the
# disjuncts of Receive, DuplicateMessage, DropMessage
COVERAGE_ACTIONS = ("Init", "Restart", "Timeout", "RequestVote", "BecomeLeader", "ClientRequest",
                    "AdvanceCommitIndex", "AppendEntries", "UpdateTerm", "Receive:RequestVoteRequest",
                    "Receive:RequestVoteResponse", "Receive:AppendEntriesRequest",
                    "Receive:AppendEntriesResponse", "DuplicateMessage", "DropMessage")
FAMILIES = ("Restart", "Timeout", "RequestVote", "BecomeLeader", "ClientRequest",
            "AdvanceCommitIndex", "AppendEntries", "Receive", "DuplicateMessage",
            "DropMessage")
ERRORS = {-22: "EINVAL", -12: "ENOMEM", -5: "HIP", -28: "CAPACITY", -19: "NOGPU",
          -74: "PARSE", -71: "STATE", -61: "IO"}


class Config(C.Structure):
    _fields_ = [("n_servers", C.c_int32), ("n_values", C.c_int32), ("max_term", C.c_int32),
                ("max_log_len", C.c_int32), ("max_msgs", C.c_int32), ("max_dup", C.c_int32),
                ("flags", C.c_uint32), ("invariants", C.c_uint32), ("device", C.c_int32),
                ("max_depth", C.c_int32), ("state_capacity", C.c_uint64), ("seed", C.c_uint64),
                ("device_window", C.c_uint64), ("set_bytes", C.c_uint64)]


class Result(C.Structure):
    _fields_ = [("generated", C.c_uint64), ("distinct", C.c_uint64), ("left_on_queue", C.c_uint64),
                ("depth", C.c_int32), ("violated_inv", C.c_int32), ("violation_depth", C.c_int32),
                ("deadlock", C.c_int32), ("collision_probability", C.c_double),
                ("seconds", C.c_double), ("expand_kernel_seconds", C.c_double),
                ("expand_launches", C.c_uint64), ("probes", C.c_uint64),
                ("collisions", C.c_uint64), ("verified", C.c_uint64),
                ("keys_sent", C.c_uint64), ("states_sent", C.c_uint64), ("chunks", C.c_uint64),
                ("exchange_seconds", C.c_double), ("stored_here", C.c_uint64),
                ("spilled", C.c_uint64), ("spills", C.c_uint64), ("spill_seconds", C.c_double),
                ("parked", C.c_uint64), ("exchange_wait_seconds", C.c_double),
                ("spill_links_on_device", C.c_int32), ("pad2", C.c_int32),
                ("verified_spilled", C.c_uint64), ("set_slots", C.c_uint64)]


class LevelStats(C.Structure):
    _fields_ = [("level", C.c_int32), ("pad", C.c_int32), ("generated", C.c_uint64),
                ("distinct", C.c_uint64), ("new_states", C.c_uint64), ("seconds", C.c_double)]


class Entry(C.Structure):
    _fields_ = [("term", C.c_int32), ("value", C.c_int32)]


class MsgView(C.Structure):
    _fields_ = [("mtype", C.c_int32), ("mterm", C.c_int32), ("msource", C.c_int32),
                ("mdest", C.c_int32), ("mlastLogTerm", C.c_int32), ("mlastLogIndex", C.c_int32),
                ("mvoteGranted", C.c_int32), ("mlog_len", C.c_int32), ("mlog", Entry * VIEW_LOG),
                ("mprevLogIndex", C.c_int32), ("mprevLogTerm", C.c_int32),
                ("mentries_len", C.c_int32), ("mentries", Entry * 1), ("mcommitIndex", C.c_int32),
                ("msuccess", C.c_int32), ("mmatchIndex", C.c_int32), ("count", C.c_int32)]


class StateView(C.Structure):
    _fields_ = [("n_servers", C.c_int32), ("n_msgs", C.c_int32),
                ("currentTerm", C.c_int32 * MAX_SERVERS), ("state", C.c_int32 * MAX_SERVERS),
                ("votedFor", C.c_int32 * MAX_SERVERS), ("commitIndex", C.c_int32 * MAX_SERVERS),
                ("log_len", C.c_int32 * MAX_SERVERS),
                ("log", (Entry * VIEW_LOG) * MAX_SERVERS),
                ("votesResponded", C.c_uint32 * MAX_SERVERS),
                ("votesGranted", C.c_uint32 * MAX_SERVERS),
                ("nextIndex", (C.c_int32 * MAX_SERVERS) * MAX_SERVERS),
                ("matchIndex", (C.c_int32 * MAX_SERVERS) * MAX_SERVERS),
                ("msgs", MsgView * VIEW_MSGS)]


class SuccView(C.Structure):
    _fields_ = [("parent", C.c_uint64), ("family", C.c_int32), ("instance", C.c_int32),
                ("in_constraint", C.c_int32), ("pad", C.c_int32), ("fingerprint", C.c_uint64),
                ("state", StateView)]


class SimConfig(C.Structure):
    _fields_ = [("behaviours", C.c_uint64), ("depth", C.c_int32), ("smoke_k", C.c_int32),
                ("smoke_nat", C.c_int32), ("mode", C.c_int32), ("seed", C.c_uint64)]


class SimResult(C.Structure):
    _fields_ = [("behaviours", C.c_uint64), ("steps", C.c_uint64), ("init_states", C.c_uint64),
                ("truncated", C.c_uint64), ("deadlocked", C.c_uint64), ("violated_inv", C.c_int32),
                ("violation_depth", C.c_int32), ("violation_behaviour", C.c_uint64),
                ("seconds", C.c_double), ("kernel_seconds", C.c_double)]


PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.POINTER(LevelStats), C.c_void_p)
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p,
                           C.POINTER(C.c_uint64))
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)


class Coverage(C.Structure):
    _fields_ = [("generated", C.c_uint64 * len(COVERAGE_ACTIONS)),
                ("distinct", C.c_uint64 * len(COVERAGE_ACTIONS))]


class Violations(C.Structure):
    _fields_ = [("states", C.c_uint64), ("first", C.c_uint64 * INV_COUNT), ("each", C.c_uint64 * INV_COUNT),
                ("depth", C.c_int32 * INV_COUNT)]


NO_STATE = (1 << 64) - 1  # RMC_NO_STATE: rmc_find_states found no stored state with the key


class Edge(C.Structure):
    """rmc_edge: one transition of the state graph; src and dst are store indices."""
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("family", C.c_int32), ("instance", C.c_int32)]


class Transport(C.Structure):
    _fields_ = [("user", C.c_void_p), ("alltoallv", ALLTOALLV_FN), ("allgather", ALLGATHER_FN)]

# Every symbol include/rmc.h declares (checked by tests/test_abi.py).
EXPORTS = ("rmc_create", "rmc_destroy", "rmc_last_error", "rmc_version", "rmc_run_bfs",
           "rmc_get_result", "rmc_trace", "rmc_state_bytes", "rmc_expand",
           "rmc_config_from_files", "rmc_probe_bench", "rmc_rccl_unique_id", "rmc_shard",
           "rmc_set_seed", "rmc_simulate", "rmc_sim_replay", "rmc_set_fp_bits",
           "rmc_sim_config_from_files", "rmc_checkpoint", "rmc_recover", "rmc_model_from_files",
           "rmc_action_location", "rmc_smoke_init", "rmc_get_coverage", "rmc_coverage_action",
           "rmc_check_states", "rmc_state_keys", "rmc_get_violations", "rmc_trace_violation",
           "rmc_get_levels", "rmc_read_states", "rmc_find_states", "rmc_graph_edges",
           "rmc_predicates_from_files", "rmc_predicates_free", "rmc_predicates_count", "rmc_predicates_name",
           "rmc_set_predicates", "rmc_eval_predicates", "rmc_predicate_error",
           "rmc_constraints_from_files", "rmc_set_constraints", "rmc_constraint_error",
           "rmc_actions_from_files", "rmc_set_actions", "rmc_eval_actions", "rmc_action_violation")

_lib = None


def native():
    """Load lib/librmc.so (built by `make -C raft.tla_amd`); raise if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"librmc.so not built: {LIB_PATH} (run __graft_entry__.build())")
        lib = C.CDLL(LIB_PATH)
        lib.rmc_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
        lib.rmc_create.restype = C.c_int
        lib.rmc_destroy.argtypes = [C.c_void_p]
        lib.rmc_destroy.restype = None
        lib.rmc_last_error.argtypes = [C.c_void_p]
        lib.rmc_last_error.restype = C.c_char_p
        lib.rmc_version.argtypes = []
        lib.rmc_version.restype = C.c_char_p
        lib.rmc_run_bfs.argtypes = [C.c_void_p, PROGRESS_FN, C.c_void_p]
        lib.rmc_run_bfs.restype = C.c_int
        lib.rmc_get_result.argtypes = [C.c_void_p, C.POINTER(Result)]
        lib.rmc_get_result.restype = C.c_int
        lib.rmc_trace.argtypes = [C.c_void_p, C.POINTER(StateView), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)]
        lib.rmc_trace.restype = C.c_int
        lib.rmc_state_bytes.argtypes = [C.POINTER(Config)]
        lib.rmc_state_bytes.restype = C.c_size_t
        lib.rmc_expand.argtypes = [C.c_void_p, C.POINTER(StateView), C.c_size_t,
                                   C.POINTER(SuccView), C.c_size_t, C.POINTER(C.c_size_t)]
        lib.rmc_expand.restype = C.c_int
        lib.rmc_config_from_files.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Config),
                                              C.c_char_p, C.c_size_t]
        lib.rmc_config_from_files.restype = C.c_int
        lib.rmc_sim_config_from_files.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Config),
                                                  C.POINTER(SimConfig), C.c_char_p, C.c_size_t]
        lib.rmc_sim_config_from_files.restype = C.c_int
        lib.rmc_model_from_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32,
                                             C.POINTER(Config), C.POINTER(SimConfig), C.c_char_p,
                                             C.c_size_t]
        lib.rmc_model_from_files.restype = C.c_int
        lib.rmc_action_location.argtypes = [C.c_char_p, C.POINTER(C.c_int32)]
        lib.rmc_action_location.restype = C.c_int
        lib.rmc_smoke_init.argtypes = [C.POINTER(Config), C.POINTER(SimConfig), C.POINTER(StateView),
                                       C.c_size_t, C.POINTER(C.c_size_t)]
        lib.rmc_smoke_init.restype = C.c_int
        lib.rmc_checkpoint.argtypes = [C.c_void_p, C.c_char_p]
        lib.rmc_checkpoint.restype = C.c_int
        lib.rmc_recover.argtypes = [C.c_void_p, C.c_char_p]
        lib.rmc_recover.restype = C.c_int
        lib.rmc_probe_bench.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_int,
                                        C.POINTER(C.c_double)]
        lib.rmc_probe_bench.restype = C.c_int
        lib.rmc_rccl_unique_id.argtypes = [C.c_char_p]
        lib.rmc_rccl_unique_id.restype = C.c_int
        lib.rmc_shard.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.POINTER(Transport),
                                  C.c_uint64, C.c_uint64]
        lib.rmc_shard.restype = C.c_int
        lib.rmc_set_seed.argtypes = [C.c_void_p, C.c_uint64]
        lib.rmc_set_seed.restype = C.c_int
        lib.rmc_set_fp_bits.argtypes = [C.c_void_p, C.c_int32]
        lib.rmc_set_fp_bits.restype = C.c_int
        lib.rmc_simulate.argtypes = [C.c_void_p, C.POINTER(SimConfig), C.POINTER(SimResult)]
        lib.rmc_simulate.restype = C.c_int
        lib.rmc_sim_replay.argtypes = [C.c_void_p, C.POINTER(SimConfig), C.c_uint64,
                                       C.POINTER(StateView), C.c_size_t, C.POINTER(C.c_size_t)]
        lib.rmc_sim_replay.restype = C.c_int
        lib.rmc_get_coverage.argtypes = [C.c_void_p, C.POINTER(Coverage)]
        lib.rmc_get_coverage.restype = C.c_int
        lib.rmc_coverage_action.argtypes = [C.c_int32]
        lib.rmc_coverage_action.restype = C.c_char_p
        lib.rmc_get_violations.argtypes = [C.c_void_p, C.POINTER(Violations)]
        lib.rmc_get_violations.restype = C.c_int
        lib.rmc_trace_violation.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(StateView), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)]
        lib.rmc_trace_violation.restype = C.c_int
        lib.rmc_check_states.argtypes = [C.c_void_p, C.POINTER(StateView), C.c_size_t, C.c_uint32,
                                         C.POINTER(C.c_int32)]
        lib.rmc_check_states.restype = C.c_int
        lib.rmc_state_keys.argtypes = [C.c_void_p, C.POINTER(StateView), C.c_size_t, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]
        lib.rmc_state_keys.restype = C.c_int
        lib.rmc_get_levels.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_size_t)]
        lib.rmc_get_levels.restype = C.c_int
        lib.rmc_read_states.argtypes = [C.c_void_p, C.c_uint64, C.c_size_t, C.POINTER(StateView),
                                        C.POINTER(C.c_uint64)]
        lib.rmc_read_states.restype = C.c_int
        lib.rmc_find_states.argtypes = [C.c_void_p, C.POINTER(StateView), C.c_size_t, C.POINTER(C.c_uint64)]
        lib.rmc_find_states.restype = C.c_int
        lib.rmc_graph_edges.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(Edge), C.c_size_t,
                                        C.POINTER(C.c_size_t)]
        lib.rmc_graph_edges.restype = C.c_int
        lib.rmc_predicates_from_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32,
                                                  C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
        lib.rmc_predicates_from_files.restype = C.c_int
        lib.rmc_predicates_free.argtypes = [C.c_void_p]
        lib.rmc_predicates_free.restype = None
        lib.rmc_predicates_count.argtypes = [C.c_void_p]
        lib.rmc_predicates_count.restype = C.c_int
        lib.rmc_predicates_name.argtypes = [C.c_void_p, C.c_int]
        lib.rmc_predicates_name.restype = C.c_char_p
        lib.rmc_set_predicates.argtypes = [C.c_void_p, C.c_void_p]
        lib.rmc_set_predicates.restype = C.c_int
        lib.rmc_eval_predicates.argtypes = [C.c_void_p, C.POINTER(StateView), C.c_size_t, C.POINTER(C.c_uint8)]
        lib.rmc_eval_predicates.restype = C.c_int
        lib.rmc_predicate_error.argtypes = [C.c_void_p]
        lib.rmc_predicate_error.restype = C.c_int
        lib.rmc_constraints_from_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32,
                                                   C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
        lib.rmc_constraints_from_files.restype = C.c_int
        lib.rmc_set_constraints.argtypes = [C.c_void_p, C.c_void_p]
        lib.rmc_set_constraints.restype = C.c_int
        lib.rmc_actions_from_files.argtypes = lib.rmc_predicates_from_files.argtypes
        lib.rmc_actions_from_files.restype = C.c_int
        lib.rmc_set_actions.argtypes = [C.c_void_p, C.c_void_p]
        lib.rmc_set_actions.restype = C.c_int
        lib.rmc_eval_actions.argtypes = [C.c_void_p, C.POINTER(StateView), C.POINTER(StateView), C.c_size_t,
                                         C.POINTER(C.c_uint8)]
        lib.rmc_eval_actions.restype = C.c_int
        lib.rmc_action_violation.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.rmc_action_violation.restype = C.c_int
        lib.rmc_constraint_error.argtypes = [C.c_void_p]
        lib.rmc_constraint_error.restype = C.c_int
        _lib = lib
    return _lib


class RmcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rmc error {code} ({ERRORS.get(code, '?')}): {msg}")
        self.code = code


def make_config(n_servers=3, n_values=2, max_term=2, max_log_len=1, max_msgs=2, max_dup=1,
                symmetry=False, bug_quorum=False, invariants=INV_TYPEOK, check_deadlock=True,
                device=0, max_depth=0, state_capacity=0, verify_states=False, spill=False, device_window=0,
                set_bytes=0, coverage=False, continue_=False):
    flags = (FLAG_SYMMETRY if symmetry else 0) | (FLAG_BUG_QUORUM if bug_quorum else 0) | \
        (FLAG_CHECK_DEADLOCK if check_deadlock else 0) | (FLAG_VERIFY_STATES if verify_states else 0) | \
        (FLAG_SPILL if spill else 0) | (FLAG_COVERAGE if coverage else 0) | (FLAG_CONTINUE if continue_ else 0)
    return Config(n_servers, n_values, max_term, max_log_len, max_msgs, max_dup, flags,
                  invariants, device, max_depth, state_capacity, 0, device_window, set_bytes)


class Predicates:
    """The model-defined invariants of a model, compiled (rmc_predicates_from_files): the
    INVARIANTs of its .cfg that are none of the ten compiled-in ones, in cfg order.
    `names`: their names; predicate p is bit INV_USER0 << p of Result.violated_inv."""

    _from_files = "rmc_predicates_from_files"

    def __init__(self, cfg_path, tla_path=None, raft_path=None, builtin_raft=False, depth_bounded=False, options=0):
        self.lib = native()
        self.handle = C.c_void_p()
        err = C.create_string_buffer(4096)
        opts = (FRONT_BUILTIN_RAFT if builtin_raft else 0) | (FRONT_DEPTH_BOUNDED if depth_bounded else 0) | options
        rc = getattr(self.lib, self._from_files)(cfg_path.encode(), tla_path.encode() if tla_path else None,
                                                 raft_path.encode() if raft_path else None, opts,
                                                 C.byref(self.handle), err, 4096)
        if rc:
            raise RmcError(rc, err.value.decode())
        self.names = [self.lib.rmc_predicates_name(self.handle, p).decode()
                      for p in range(self.lib.rmc_predicates_count(self.handle))]

    def __len__(self):
        return len(self.names)

    def name_of(self, violated_inv):
        """The name behind a Result.violated_inv user bit (None for a compiled-in bit)."""
        for p, name in enumerate(self.names):
            if violated_inv == INV_USER0 << p:
                return name
        return None

    def close(self):
        if self.handle:
            self.lib.rmc_predicates_free(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        self.close()


class Constraints(Predicates):
    """The residual conjuncts of a model's CONSTRAINTs, compiled (rmc_constraints_from_files):
    every top-level conjunct that is none of the four bounds, in order.  `names`: per
    residual the CONSTRAINT of the .cfg it came from.  Empty: the model has none."""
    _from_files = "rmc_constraints_from_files"


class Actions(Predicates):
    """The action properties of a model, compiled (rmc_actions_from_files): the PROPERTY names
    of its .cfg whose definition is [][A]_vars, in cfg order.  Property p is bit
    ACT_USER0 << p of Result.violated_inv.  Empty: the model has none."""
    _from_files = "rmc_actions_from_files"

    def name_of(self, violated_inv):
        for p, name in enumerate(self.names):
            if violated_inv == ACT_USER0 << p:
                return name
        return None


def load_model(cfg_path, tla_path=None, raft_path=None, builtin_raft=False, depth_bounded=False, predicates=False,
               constraints=False, actions=False):
    """(Config, provenance notes, Predicates or None): rmc_model_from_files for a BFS model;
    predicates=True accepts INVARIANTs of the model's own (RMC_FRONT_PREDICATES) and
    compiles them — hand them to Checker.set_predicates.  constraints=True accepts
    CONSTRAINT conjuncts that are no bound (RMC_FRONT_CONSTRAINTS), compiles them, and
    returns a fourth value, the Constraints — hand them to Checker.set_constraints.
    actions=True accepts PROPERTY names of the form [][A]_vars (RMC_FRONT_ACTIONS), compiles
    them, and returns the Actions as one more, last value — hand them to Checker.set_actions."""
    cfg, _sc, notes = model_from_files(cfg_path, tla_path, raft_path, builtin_raft, depth_bounded=depth_bounded,
                                       predicates=predicates, constraints=constraints, actions=actions)
    every = (FRONT_CONSTRAINTS if constraints else 0) | (FRONT_PREDICATES if predicates else 0) | \
        (FRONT_ACTIONS if actions else 0)
    preds = Predicates(cfg_path, tla_path, raft_path, builtin_raft, depth_bounded, every) if predicates else None
    out = [cfg, notes, preds]
    if constraints:
        out.append(Constraints(cfg_path, tla_path, raft_path, builtin_raft, depth_bounded, every))
    if actions:
        out.append(Actions(cfg_path, tla_path, raft_path, builtin_raft, depth_bounded, every))
    return tuple(out)


def model_from_files(cfg_path, tla_path=None, raft_path=None, builtin_raft=False, simulate=False,
                     depth_bounded=False, predicates=False, constraints=False, actions=False):
    """rmc_model_from_files: (Config, SimConfig or None, provenance notes).
    Raises RmcError naming the construct when the model is not the compiled-in
    raft.tla (with its recognised bug variant, bounds and invariants).
    depth_bounded: the caller sets max_depth (TLC -depth), so fields without a
    CONSTRAINT are accepted at the packed capacity (RMC_FLAG_UNBOUNDED_*)."""
    lib = native()
    cfg, sc = Config(), SimConfig()
    info = C.create_string_buffer(4096)
    opts = (FRONT_BUILTIN_RAFT if builtin_raft else 0) | (FRONT_SIMULATE if simulate else 0) | \
        (FRONT_DEPTH_BOUNDED if depth_bounded else 0) | (FRONT_PREDICATES if predicates else 0) | \
        (FRONT_CONSTRAINTS if constraints else 0) | (FRONT_ACTIONS if actions else 0)
    rc = lib.rmc_model_from_files(cfg_path.encode(), tla_path.encode() if tla_path else None,
                                  raft_path.encode() if raft_path else None, opts, C.byref(cfg),
                                  C.byref(sc) if simulate else None, info, 4096)
    if rc:
        raise RmcError(rc, info.value.decode())
    return cfg, (sc if simulate else None), info.value.decode()


def config_from_files(cfg_path, tla_path=None, raft_path=None, builtin_raft=False):
    return model_from_files(cfg_path, tla_path, raft_path, builtin_raft)[0]


def sim_config_from_files(cfg_path, tla_path=None, raft_path=None, builtin_raft=False):
    """(Config, SimConfig) of a simulation model (Smokeraft.cfg: Init <- SmokeInit)."""
    cfg, sc, _ = model_from_files(cfg_path, tla_path, raft_path, builtin_raft, simulate=True)
    return cfg, sc


def smoke_init(cfg, smoke_k, smoke_nat=2, seed=0):
    """The SmokeInit initial states rmc_simulate would draw (host only)."""
    sc = SimConfig(1, 100, smoke_k, smoke_nat, 0, seed)
    n = C.c_size_t()
    rc = native().rmc_smoke_init(C.byref(cfg), C.byref(sc), None, 0, C.byref(n))
    if rc:
        raise RmcError(rc, "rmc_smoke_init failed")
    st = (StateView * n.value)()
    rc = native().rmc_smoke_init(C.byref(cfg), C.byref(sc), st, n.value, C.byref(n))
    if rc:
        raise RmcError(rc, "rmc_smoke_init failed")
    return list(st)


def rccl_unique_id() -> bytes:
    """rmc_rccl_unique_id: the 128-byte id rank 0 hands to every rank's rmc_shard."""
    buf = C.create_string_buffer(128)
    rc = native().rmc_rccl_unique_id(buf)
    if rc:
        raise RmcError(rc, "rmc_rccl_unique_id failed")
    return buf.raw


def action_location(action):
    """(line, col, line, col) of an action of Next in raft.tla (TLC's trace headers)."""
    out = (C.c_int32 * 4)()
    rc = native().rmc_action_location(action.encode(), out)
    if rc:
        raise RmcError(rc, f"no action {action!r}")
    return tuple(out)


def probe_bench(device=0, table_bytes=64 << 30, accesses=1 << 31, mode=0):
    """Random 8-byte probe (mode 0) / CAS (mode 1) rate over a table of
    table_bytes: the roofline ceiling R_max of the fingerprint set."""
    rate = C.c_double()
    rc = native().rmc_probe_bench(device, table_bytes, accesses, mode, C.byref(rate))
    if rc:
        raise RmcError(rc, "rmc_probe_bench failed")
    return rate.value


class _ProgressRows(list):
    """What run() leaves in Checker.levels: the progress callback's rows, as before —
    and, called, Checker.levels() (the attribute has shadowed the method since run())."""

    def __init__(self, rows, checker):
        super().__init__(rows)
        self._checker = checker

    def __call__(self):
        return Checker.levels(self._checker)


class Checker:
    """One model-checking context on one GPU (rmc_ctx)."""

    def __init__(self, cfg: Config):
        self.lib = native()
        self.cfg = cfg
        self.ctx = C.c_void_p()
        rc = self.lib.rmc_create(C.byref(cfg), C.byref(self.ctx))
        if rc:
            raise RmcError(rc, "rmc_create failed (see stderr)")

    def close(self):
        if self.ctx:
            self.lib.rmc_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc:
            raise RmcError(rc, self.lib.rmc_last_error(self.ctx).decode())

    def run(self, progress=None, record_levels=True) -> Result:
        """rmc_run_bfs.  record_levels=False (and no progress callback) passes
        no callback at all, as a Java caller without a progress listener
        would: a sharded search then skips the per-level stop vote."""
        levels = []

        def cb(p, _u):
            s = p.contents
            levels.append((s.level, s.generated, s.distinct, s.new_states, s.seconds))
            return int(bool(progress and progress(s)))

        fn = PROGRESS_FN(cb) if (record_levels or progress) else PROGRESS_FN()
        self._check(self.lib.rmc_run_bfs(self.ctx, fn, None))
        res = Result()
        self._check(self.lib.rmc_get_result(self.ctx, C.byref(res)))
        self.levels = _ProgressRows(levels, self)
        return res

    def simulate(self, behaviours=1 << 20, depth=100, smoke_k=2, smoke_nat=2, seed=0, mode=0) -> SimResult:
        """TLC -simulate over Smokeraft-style initial states (rmc_simulate);
        mode 0 = RMC_SIM_WITHIN_CAPACITY, 1 = RMC_SIM_TRUNCATE, 2 = RMC_SIM_TLC (TLC's
        draw: an action, then a successor; the wide layout only)."""
        sc = SimConfig(behaviours, depth, smoke_k, smoke_nat, mode, seed)
        out = SimResult()
        self._check(self.lib.rmc_simulate(self.ctx, C.byref(sc), C.byref(out)))
        return out

    def sim_replay(self, behaviour, behaviours=1 << 20, depth=100, smoke_k=2, smoke_nat=2, seed=0, mode=0):
        """States of one behaviour of the same simulation (rmc_sim_replay)."""
        sc = SimConfig(behaviours, depth, smoke_k, smoke_nat, mode, seed)
        st = (StateView * depth)()
        n = C.c_size_t()
        self._check(self.lib.rmc_sim_replay(self.ctx, C.byref(sc), behaviour, st, depth, C.byref(n)))
        return [st[k] for k in range(min(n.value, depth))]

    def shard(self, rank: int, world: int, rccl_id: bytes | None = None, transport=None,
              keys_per_dest: int = 0, sent_cache_slots: int = 0):
        """rmc_shard: make this ctx rank `rank` of `world`.  RCCL when rccl_id
        (from rccl_unique_id() on rank 0) is given, else `transport` (a
        Transport, e.g. rmc.dist.GlooTransport().struct)."""
        self._shard_keep = transport  # the callbacks must outlive the ctx
        st = getattr(transport, "struct", transport)
        self._check(self.lib.rmc_shard(self.ctx, rank, world, rccl_id,
                                       C.byref(st) if st is not None else None,
                                       keys_per_dest, sent_cache_slots))

    def checkpoint(self, path: str):
        """Write the stopped search to `path` (rmc_checkpoint; TLC -checkpoint)."""
        self._check(self.lib.rmc_checkpoint(self.ctx, path.encode()))

    def recover(self, path: str):
        """Load a checkpoint; the next run() continues it (rmc_recover; TLC -recover)."""
        self._check(self.lib.rmc_recover(self.ctx, path.encode()))

    def set_fp_bits(self, bits: int):
        """Verification-mode test hook: keep only `bits` fingerprint bits (rmc_set_fp_bits)."""
        self._check(self.lib.rmc_set_fp_bits(self.ctx, bits))

    def set_seed(self, seed: int):
        """Fingerprint salt for the next run (rmc_set_seed)."""
        self._check(self.lib.rmc_set_seed(self.ctx, seed))

    def coverage(self):
        """rmc_get_coverage after a run() on a ctx made with coverage=True:
        {action: (generated, distinct)} in the order of COVERAGE_ACTIONS."""
        cv = Coverage()
        self._check(self.lib.rmc_get_coverage(self.ctx, C.byref(cv)))
        return {a: (cv.generated[k], cv.distinct[k]) for k, a in enumerate(COVERAGE_ACTIONS)}

    def violations(self) -> Violations:
        """rmc_get_violations after a run() on a ctx made with continue_=True (TLC
        -continue): states, and per invariant r (bit 1 << r) first[r], each[r], depth[r]."""
        v = Violations()
        self._check(self.lib.rmc_get_violations(self.ctx, C.byref(v)))
        return v

    def trace_violation(self, bit):
        """rmc_trace_violation: trace() to the least-index stored state that violates
        the invariant `bit` (one INV_* bit of the config's mask) checked alone."""
        n = C.c_size_t()
        self._check(self.lib.rmc_trace_violation(self.ctx, bit, None, None, None, 0, C.byref(n)))
        st = (StateView * n.value)()
        fam = (C.c_int32 * n.value)()
        inst = (C.c_int32 * n.value)()
        self._check(self.lib.rmc_trace_violation(self.ctx, bit, st, fam, inst, n.value, C.byref(n)))
        return [(fam[k], inst[k], st[k]) for k in range(n.value)]

    def result(self) -> Result:
        res = Result()
        self._check(self.lib.rmc_get_result(self.ctx, C.byref(res)))
        return res

    def trace(self):
        n = C.c_size_t()
        self._check(self.lib.rmc_trace(self.ctx, None, None, None, 0, C.byref(n)))
        st = (StateView * n.value)()
        fam = (C.c_int32 * n.value)()
        inst = (C.c_int32 * n.value)()
        self._check(self.lib.rmc_trace(self.ctx, st, fam, inst, n.value, C.byref(n)))
        return [(fam[k], inst[k], st[k]) for k in range(n.value)]

    def expand(self, views):
        arr = (StateView * len(views))(*views)
        lanes_max = 5 + 5 + 25 + 5 + 10 + 5 + 25 + 3 * VIEW_MSGS
        cap = max(1, len(views) * lanes_max)
        out = (SuccView * cap)()
        n = C.c_size_t()
        self._check(self.lib.rmc_expand(self.ctx, arr, len(views), out, cap, C.byref(n)))
        return [out[k] for k in range(min(n.value, cap))]

    def check_states(self, views, invariants=0):
        """rmc_check_states: per view 0, or the RMC_INV_* bit of the first invariant of
        the mask (0 = the ctx's own) that the device code finds violated.  `views`:
        a sequence of StateView, or a ctypes array of them (passed as it is)."""
        arr = views if isinstance(views, C.Array) else (StateView * len(views))(*views)
        out = (C.c_int32 * len(views))()
        self._check(self.lib.rmc_check_states(self.ctx, arr, len(views), invariants, out))
        return list(out)

    def state_keys(self, views, ref=None):
        """rmc_state_keys: per view the 64-bit key the search would insert for it
        (under symmetry=True the canonical key of its orbit).  With ref (one index
        into views per view): (keys, same), same[t] = 1 iff verification's
        comparison finds view t equal to the stored form of view ref[t].  `views`:
        a sequence of StateView, or a ctypes array of them (passed as it is)."""
        arr = views if isinstance(views, C.Array) else (StateView * len(views))(*views)
        keys = (C.c_uint64 * len(views))()
        if ref is None:
            self._check(self.lib.rmc_state_keys(self.ctx, arr, len(views), keys, None, None))
            return list(keys)
        assert len(ref) == len(views)
        refs = (C.c_uint32 * len(views))(*ref)
        same = (C.c_uint8 * len(views))()
        self._check(self.lib.rmc_state_keys(self.ctx, arr, len(views), keys, refs, same))
        return list(keys), list(same)

    # ---- model-defined invariants (rmc.h "model-defined invariants") ----
    def set_predicates(self, preds):
        """rmc_set_predicates: run() then checks the compiled predicates (a Predicates) on
        every stored state; None removes them.  The ctx keeps its own copy."""
        self._check(self.lib.rmc_set_predicates(self.ctx, preds.handle if preds is not None else None))
        self._pred_names = list(preds.names) if preds is not None else []

    def eval_predicates(self, views):
        """rmc_eval_predicates: per view the verdict of every predicate, in order
        (PRED_HOLDS, PRED_VIOLATED, PRED_ERROR), by the device interpreter.  `views`: a
        sequence of StateView, or a ctypes array of them (passed as it is)."""
        arr = views if isinstance(views, C.Array) else (StateView * len(views))(*views)
        np_ = len(getattr(self, "_pred_names", []))
        out = (C.c_uint8 * max(1, len(views) * np_))()
        self._check(self.lib.rmc_eval_predicates(self.ctx, arr, len(views), out))
        return [tuple(out[t * np_:(t + 1) * np_]) for t in range(len(views))]

    def predicate_name(self, violated_inv):
        """The name of the predicate behind a Result.violated_inv user bit, else None."""
        for p, name in enumerate(getattr(self, "_pred_names", [])):
            if violated_inv == INV_USER0 << p:
                return name
        return None

    def predicate_error(self):
        """rmc_predicate_error: True if the violation run() reported is an evaluation error."""
        return bool(self.lib.rmc_predicate_error(self.ctx))

    # ---- model-defined constraints (rmc.h "model-defined constraints") ----
    def set_constraints(self, cons):
        """rmc_set_constraints: run() then keeps only the states on which every compiled
        residual (a Constraints) holds; None removes them.  The ctx keeps its own copy."""
        self._check(self.lib.rmc_set_constraints(self.ctx, cons.handle if cons is not None else None))

    def constraint_error(self):
        """rmc_constraint_error: 1 + the residual whose evaluation error stopped run(), else 0."""
        return self.lib.rmc_constraint_error(self.ctx)

    # ---- action properties (rmc.h "action properties") ----
    def set_actions(self, acts):
        """rmc_set_actions: run() then checks the compiled action properties (an Actions) on
        every transition; None removes them.  The ctx keeps its own copy."""
        self._check(self.lib.rmc_set_actions(self.ctx, acts.handle if acts is not None else None))
        self._act_names = list(acts.names) if acts is not None else []

    def eval_actions(self, pairs):
        """rmc_eval_actions: per pair (current StateView, next StateView) the verdict of every
        property, in order (PRED_HOLDS, PRED_VIOLATED, PRED_ERROR), by the device interpreter,
        with the stutter rule applied."""
        cur = (StateView * len(pairs))(*[p[0] for p in pairs])
        nxt = (StateView * len(pairs))(*[p[1] for p in pairs])
        np_ = len(getattr(self, "_act_names", []))
        out = (C.c_uint8 * max(1, len(pairs) * np_))()
        self._check(self.lib.rmc_eval_actions(self.ctx, cur, nxt, len(pairs), out))
        return [tuple(out[t * np_:(t + 1) * np_]) for t in range(len(pairs))]

    def action_violation(self):
        """rmc_action_violation: the transition run() reported, as a dict (property, name,
        src_index, family, instance, is_error); RmcError(E_STATE) when it reported none."""
        prop, fam, inst, err = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        src = C.c_uint64()
        self._check(self.lib.rmc_action_violation(self.ctx, C.byref(prop), C.byref(src), C.byref(fam), C.byref(inst),
                                                  C.byref(err)))
        names = getattr(self, "_act_names", [])
        return {"property": prop.value, "name": names[prop.value] if prop.value < len(names) else None,
                "src_index": src.value, "family": fam.value, "instance": inst.value, "is_error": bool(err.value)}

    # ---- the state graph of the last completed run() (rmc.h "state graph export") ----
    def levels(self):
        """rmc_get_levels: starts[l] = the store index of the first state of level
        l + 1; the last entry = distinct."""
        n = C.c_size_t()
        self._check(self.lib.rmc_get_levels(self.ctx, None, 0, C.byref(n)))
        starts = (C.c_uint64 * n.value)()
        self._check(self.lib.rmc_get_levels(self.ctx, starts, n.value, C.byref(n)))
        return list(starts)

    def read_states(self, first, n, keys=False):
        """rmc_read_states: the stored states [first, first + n) as a ctypes array of
        StateView; keys=True: (states, keys), the key the search inserted for each."""
        st = (StateView * n)()
        ks = (C.c_uint64 * n)() if keys else None
        self._check(self.lib.rmc_read_states(self.ctx, first, n, st, ks))
        return (st, list(ks)) if keys else st

    def find_states(self, views):
        """rmc_find_states: per view the store index of the stored state with its key
        (under symmetry=True: of its orbit's stored representative), or NO_STATE.
        `views`: a sequence of StateView, or a ctypes array of them (passed as it is)."""
        arr = views if isinstance(views, C.Array) else (StateView * len(views))(*views)
        index = (C.c_uint64 * len(views))()
        self._check(self.lib.rmc_find_states(self.ctx, arr, len(views), index))
        return list(index)

    def graph_edges(self, lo, hi, cap=None):
        """rmc_graph_edges: every edge out of the stored states [lo, hi), in (src,
        instance) order, as a ctypes array of Edge.  cap: the room offered (default:
        what the range needs); returns (edges written, n_out) then."""
        n = C.c_size_t()
        if cap is not None:
            out = (Edge * max(1, cap))()
            self._check(self.lib.rmc_graph_edges(self.ctx, lo, hi, out, cap, C.byref(n)))
            return out[:min(cap, n.value)], n.value
        self._check(self.lib.rmc_graph_edges(self.ctx, lo, hi, None, 0, C.byref(n)))
        out = (Edge * max(1, n.value))()
        self._check(self.lib.rmc_graph_edges(self.ctx, lo, hi, out, n.value, C.byref(n)))
        return out[:n.value]
