// dump_check.cpp — rmc-tlc -dump's writers (raft.tla_amd/csrc/rmc_dump.cpp) on a hand-made
// five-node graph, host only: `dump_check dot|dotlabels|states|badedge` writes to stdout what
// the writer produces (tests/test_graph_native.py holds the expected text).
//
// The graph: levels {n0}, {n1, n2}, {n3, n4}; keys chosen so that the (level, id) order differs
// from the array order (a key above 2^63 is a negative id), a label with a quote and a
// backslash, a self-loop (a stutter), and two edges between the same two nodes.
#include <cstdio>
#include <cstring>

#include "rmc_dump.h"

int main(int argc, char** argv) {
    using rmc_dump::Edge;
    using rmc_dump::Node;
    if (argc != 2) return 2;
    const std::vector<Node> nodes = {
        {42ull, 1, "/\\ x = 0\n/\\ y = \"a\"\n"},
        {7ull, 2, "/\\ x = 1\n"},
        {0xFFFFFFFFFFFFFFFFull, 2, "/\\ x = 2\n"},  // id -1: before 7 in its level
        {0x8000000000000000ull, 3, "/\\ x = 3\n"},  // the least id
        {5ull, 3, "/\\ x = 4\n"},
    };
    std::vector<Edge> edges = {
        {0, 1, 1, 3}, {0, 2, 0, 0}, {1, 3, 2, 9}, {1, 3, 2, 4}, {1, 3, 1, 20},
        {2, 4, 9, 30}, {0, 0, 8, 25}, {2, 2, 7, 21},
    };
    static const char* const kFam[10] = {"Restart", "Timeout", "RequestVote", "BecomeLeader", "ClientRequest",
                                         "AdvanceCommitIndex", "AppendEntries", "Receive", "DuplicateMessage",
                                         "DropMessage"};
    bool ok;
    if (!strcmp(argv[1], "dot")) ok = rmc_dump::write_dot(stdout, nodes, edges, kFam, 10, false);
    else if (!strcmp(argv[1], "dotlabels")) ok = rmc_dump::write_dot(stdout, nodes, edges, kFam, 10, true);
    else if (!strcmp(argv[1], "states")) ok = rmc_dump::write_states(stdout, nodes);
    else if (!strcmp(argv[1], "badedge")) {  // an edge to a node that does not exist: refused, nothing written
        edges.push_back({4, 5, 0, 0});
        ok = !rmc_dump::write_dot(stdout, nodes, edges, kFam, 10, true);
    } else return 2;
    return ok ? 0 : 1;
}
