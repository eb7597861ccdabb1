// rmc_dump.cpp — the writers of `rmc-tlc -dump` (rmc_dump.h).
#include "rmc_dump.h"

#include <algorithm>
#include <cinttypes>
#include <tuple>

namespace rmc_dump {

std::string node_id(uint64_t key) {
    char buf[32];
    snprintf(buf, sizeof buf, "%" PRId64, (int64_t)key);
    return buf;
}

std::string dot_label(const std::string& text) {
    std::string s;
    size_t n = text.size();
    while (n && text[n - 1] == '\n') --n;
    for (size_t q = 0; q < n; ++q) {
        const char ch = text[q];
        if (ch == '\\') s += "\\\\";
        else if (ch == '"') s += "\\\"";
        else if (ch == '\n') s += "\\n";
        else s += ch;
    }
    return s;
}

bool write_states(FILE* f, const std::vector<Node>& nodes) {
    for (size_t k = 0; k < nodes.size(); ++k)
        if (fprintf(f, "State %zu:\n%s\n", k + 1, nodes[k].text.c_str()) < 0) return false;
    return fflush(f) == 0;
}

bool write_dot(FILE* f, const std::vector<Node>& nodes, const std::vector<Edge>& edges, const char* const* families,
               int n_families, bool actionlabels) {
    for (const Edge& e : edges)
        if (e.src >= nodes.size() || e.dst >= nodes.size() || e.family < 0 || e.family >= n_families) return false;
    auto id = [&](uint64_t ix) { return (int64_t)nodes[ix].key; };
    std::vector<size_t> no(nodes.size()), eo(edges.size());
    for (size_t q = 0; q < no.size(); ++q) no[q] = q;
    for (size_t q = 0; q < eo.size(); ++q) eo[q] = q;
    std::sort(no.begin(), no.end(), [&](size_t a, size_t b) {
        return std::make_tuple(nodes[a].level, id(a), a) < std::make_tuple(nodes[b].level, id(b), b);
    });
    std::sort(eo.begin(), eo.end(), [&](size_t a, size_t b) {
        const Edge &x = edges[a], &y = edges[b];
        return std::make_tuple(id(x.src), id(x.dst), x.family, x.instance, a) <
               std::make_tuple(id(y.src), id(y.dst), y.family, y.instance, b);
    });
    fprintf(f, "strict digraph DiskGraph {\nnodesep=0.35;\nsubgraph cluster_graph {\ncolor=\"white\";\n");
    for (size_t q : no)
        fprintf(f, "%s [label=\"%s\"%s\n", node_id(nodes[q].key).c_str(), dot_label(nodes[q].text).c_str(),
                nodes[q].level == 1 ? ",style = filled]" : "];");
    for (size_t q : eo) {
        const Edge& e = edges[q];
        if (actionlabels)
            fprintf(f, "%s -> %s [label=\"%s\"];\n", node_id(nodes[e.src].key).c_str(), node_id(nodes[e.dst].key).c_str(),
                    families[e.family]);
        else
            fprintf(f, "%s -> %s;\n", node_id(nodes[e.src].key).c_str(), node_id(nodes[e.dst].key).c_str());
    }
    for (size_t a = 0; a < no.size();) {  // one rank line per level
        size_t b = a;
        fprintf(f, "{rank = same; ");
        for (; b < no.size() && nodes[no[b]].level == nodes[no[a]].level; ++b) fprintf(f, "%s;", node_id(nodes[no[b]].key).c_str());
        fprintf(f, "}\n");
        a = b;
    }
    fprintf(f, "}\n}\n");
    return fflush(f) == 0 && !ferror(f);
}

}  // namespace rmc_dump
