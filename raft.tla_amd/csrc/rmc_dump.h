// rmc_dump.h — the writers of `rmc-tlc -dump` (TLC's -dump FILE and -dump dot[,actionlabels]
// FILE): host-only, no HIP and no rmc.h — they take the graph as arrays of nodes and edges, so
// they are tested without a device (tests/native/dump_check.cpp).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace rmc_dump {

struct Node {
    uint64_t key;      // the state's 64-bit key; its node id is the key as a signed decimal (TLC prints fingerprints)
    int level;         // BFS level, 1 = initial
    std::string text;  // the state as TLC prints it: one "/\ var = value" line per variable, '\n' after each
};
struct Edge {
    uint64_t src, dst;  // indices into the node array
    int family;         // index into the family names (the label under actionlabels)
    int instance;       // the lane: orders the edges between the same two states
};

// The node id of a key.
std::string node_id(uint64_t key);
// `text` inside a dot "label": backslashes and quotes escaped, line ends as \n, none at the end.
std::string dot_label(const std::string& text);

// TLC -dump FILE: every state as a block "State k:\n<text>\n", in the order given.
bool write_states(FILE* f, const std::vector<Node>& nodes);

// TLC -dump dot[,actionlabels] FILE:
//   strict digraph DiskGraph {
//   nodesep=0.35;
//   subgraph cluster_graph {
//   color="white";
//   <id> [label="<state>",style = filled]      initial states (level 1)
//   <id> [label="<state>"];                    the others, nodes in (level, id) order
//   <a> -> <b> [label="<family>"];             edges in (source id, destination id, family, instance)
//   <a> -> <b>;                                order; the label only with actionlabels
//   {rank = same; <id>;<id>;}                  one line per level
//   }
//   }
// Ids compare as the signed numbers they are written as.  An edge whose src or dst is not a
// node index makes the call fail before anything is written.
bool write_dot(FILE* f, const std::vector<Node>& nodes, const std::vector<Edge>& edges, const char* const* families,
               int n_families, bool actionlabels);

}  // namespace rmc_dump
