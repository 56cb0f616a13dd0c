/*
 * consent_amd_adapter.hpp -- C++ host side over the C ABI, shaped like CONSENT's operator
 * (computeConsensusReadCorrection / computeConsensusAssemblyPolishing, src/correctionMSA.h:8,10) but batched over windows.
 *
 * Header-only; needs only consent_amd.h and the shared library.  It mirrors the reference interface for this path:
 * same parameter names and meaning; the `(consensus, merCounts)` pair of the reference becomes
 * `(consensus, solid k-mers)` -- downstream code reads merCounts only through `count >= solidThresh`
 * (src/correctionAlignment.cpp:6-15).  Errors: std::runtime_error on a library error; a window whose capacity overflowed
 * comes back with `overflow = true` and an empty consensus (the caller decides what to do with it).
 */
#ifndef CONSENT_AMD_ADAPTER_HPP
#define CONSENT_AMD_ADAPTER_HPP

#include <cstdint>
#include <array>
#include <stdexcept>
#include <string>
#include <vector>

#include "consent_amd.h"

namespace consent_amd {

struct WindowConsensus {
    std::string consensus;             /* case-annotated, as the reference returns it                       */
    std::vector<uint32_t> solid_kmers; /* ascending, str2num order, count >= solidThresh in the window pile */
    bool template_fallback = false;    /* MSA empty: raw template returned (correctionMSA.cpp:34-36)        */
    bool overflow = false;
};

class Engine {
  public:
    Engine(unsigned merSize, unsigned solidThresh, unsigned commonKMers, unsigned minAnchors, unsigned maxMSA, int device = 0) : solid_(solidThresh) {
        cw_params p{merSize, solidThresh, commonKMers, minAnchors, maxMSA};
        const int rc = cw_create(&p, device, &eng_);
        if (rc != CW_OK) throw std::runtime_error(std::string("consent_amd: cw_create: ") + cw_strerror(rc));
    }
    ~Engine() { cw_destroy(eng_); }
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;

    /* piles[w] = what getAlignmentWindowsSequences returned for window w (template first, alignmentWindows.cpp:100) */
    std::vector<WindowConsensus> computeConsensus(const std::vector<std::vector<std::string>>& piles) {
        std::vector<uint32_t> wfs{0}, len, bases;
        std::vector<uint64_t> off;
        for (const auto& pile : piles) {
            for (const auto& s : pile) {
                const uint64_t words = (s.size() + 15) / 16;
                off.push_back(bases.size());
                len.push_back((uint32_t)s.size());
                bases.resize(bases.size() + words);
                if (words && cw_pack_sequence(s.data(), (uint32_t)s.size(), bases.data() + off.back(), words) < 0)
                    throw std::runtime_error("consent_amd: cw_pack_sequence failed");
            }
            wfs.push_back((uint32_t)len.size());
        }
        bases.push_back(0);
        const uint32_t W = (uint32_t)piles.size();
        std::vector<uint64_t> coff(W + 1, 0), soff(W + 1, 0);
        for (uint32_t w = 0; w < W; ++w) {
            uint64_t tpl = piles[w].empty() ? 0 : piles[w][0].size(), tot = 0;
            for (const auto& s : piles[w]) tot += s.size();
            coff[w + 1] = coff[w] + 3 * tpl + 256;
            soff[w + 1] = soff[w] + tot / (solid_ ? solid_ : 1) + 16;
        }
        std::vector<char> cons(coff[W] + 1);
        std::vector<uint32_t> clen(W), solid(soff[W] + 1), slen(W);
        std::vector<uint8_t> st(W);
        std::vector<WindowConsensus> out(W);
        if (W == 0) return out;
        cw_batch b{W, (uint32_t)len.size(), (uint64_t)bases.size() - 1, wfs.data(), len.data(), off.data(), bases.data()};
        cw_result r{cons.data(), coff.data(), clen.data(), st.data(), solid.data(), soff.data(), slen.data()};
        const int rc = cw_run(eng_, &b, &r);
        if (rc != CW_OK && rc != CW_E_CAPACITY) throw std::runtime_error(std::string("consent_amd: cw_run: ") + cw_strerror(rc));
        for (uint32_t w = 0; w < W; ++w) {
            out[w].overflow = st[w] == CW_WIN_OVERFLOW;
            out[w].template_fallback = st[w] == CW_WIN_TEMPLATE;
            if (out[w].overflow) continue;
            out[w].consensus.assign(cons.data() + coff[w], clen[w]);
            out[w].solid_kmers.assign(solid.begin() + soff[w], solid.begin() + soff[w] + slen[w]);
        }
        return out;
    }

    /* Only the POA (cw_poa_run): the consensus of every group of sequences, aligned in the order given -- one segment of the window path each.  A group that
       stopped (a member beyond 4 095 bases, a graph beyond the last tier) comes back with overflow = true and an empty consensus. */
    std::vector<WindowConsensus> poaConsensus(const std::vector<std::vector<std::string>>& groups) {
        std::vector<uint32_t> wfs{0}, len, bases;
        std::vector<uint64_t> off, coff{0};
        for (const auto& group : groups) {
            size_t longest = 0;
            for (const auto& s : group) {
                const uint64_t words = (s.size() + 15) / 16;
                off.push_back(bases.size());
                len.push_back((uint32_t)s.size());
                bases.resize(bases.size() + words);
                if (words && cw_pack_sequence(s.data(), (uint32_t)s.size(), bases.data() + off.back(), words) < 0)
                    throw std::runtime_error("consent_amd: cw_pack_sequence failed");
                if (s.size() > longest) longest = s.size();
            }
            wfs.push_back((uint32_t)len.size());
            coff.push_back(coff.back() + CW_POA_SLOT_BYTES(longest));
        }
        bases.push_back(0);
        const uint32_t G = (uint32_t)groups.size();
        std::vector<char> cons(coff[G] + 1);
        std::vector<uint32_t> clen(G);
        std::vector<uint8_t> st(G);
        std::vector<WindowConsensus> out(G);
        if (G == 0) return out;
        cw_batch b{G, (uint32_t)len.size(), (uint64_t)bases.size() - 1, wfs.data(), len.data(), off.data(), bases.data()};
        cw_result r{cons.data(), coff.data(), clen.data(), st.data(), nullptr, nullptr, nullptr};
        const int rc = cw_poa_run(eng_, &b, &r);
        if (rc != CW_OK && rc != CW_E_CAPACITY) throw std::runtime_error(std::string("consent_amd: cw_poa_run: ") + cw_strerror(rc));
        for (uint32_t g = 0; g < G; ++g) {
            out[g].overflow = st[g] == CW_WIN_OVERFLOW;
            if (!out[g].overflow) out[g].consensus.assign(cons.data() + coff[g], clen[g]);
        }
        return out;
    }

    /* Only the local alignment (cw_sw_run): every sequence of a group against the group's first.  Row [g][m] is member m of group g: the eight numbers of
       consent_amd.h (CW_SW_SCORE .. CW_SW_STATUS); [g][0] is the reference's own row (CW_SW_IS_REF).  A pair beyond a capacity has status CW_SW_STOP. */
    std::vector<std::vector<std::array<int32_t, CW_SW_ROW>>> alignToFirst(const std::vector<std::vector<std::string>>& groups, bool want_indels = false) {
        std::vector<uint32_t> wfs{0}, len, bases;
        std::vector<uint64_t> off;
        for (const auto& group : groups) {
            for (const auto& s : group) {
                const uint64_t words = (s.size() + 15) / 16;
                off.push_back(bases.size());
                len.push_back((uint32_t)s.size());
                bases.resize(bases.size() + words);
                if (words && cw_pack_sequence(s.data(), (uint32_t)s.size(), bases.data() + off.back(), words) < 0)
                    throw std::runtime_error("consent_amd: cw_pack_sequence failed");
            }
            wfs.push_back((uint32_t)len.size());
        }
        bases.push_back(0);
        std::vector<int32_t> rows(len.size() * CW_SW_ROW + 1);
        cw_batch b{(uint32_t)groups.size(), (uint32_t)len.size(), (uint64_t)bases.size() - 1, wfs.data(), len.data(), off.data(), bases.data()};
        const int rc = cw_sw_run(eng_, &b, rows.data(), want_indels ? CW_SW_WANT_INDELS : 0u);
        if (rc != CW_OK && rc != CW_E_CAPACITY) throw std::runtime_error(std::string("consent_amd: cw_sw_run: ") + cw_strerror(rc));
        std::vector<std::vector<std::array<int32_t, CW_SW_ROW>>> out(groups.size());
        for (size_t g = 0; g < groups.size(); ++g)
            for (uint32_t s = wfs[g]; s < wfs[g + 1]; ++s) {
                std::array<int32_t, CW_SW_ROW> row;
                for (int k = 0; k < CW_SW_ROW; ++k) row[k] = rows[(size_t)s * CW_SW_ROW + k];
                out[g].push_back(row);
            }
        return out;
    }

    /* The local alignment cut at the reference's window boundaries (cw_sw_cut_run): [g][m] holds the cut points of member m >= 1 of group g -- word t the
       position in the member at column t x window of the group's first sequence, so that member.substr(c[t], c[t + 1] - c[t]) is what its alignment puts
       on window t -- and [g][0] is empty.  A member that does not align gets zeros. */
    std::vector<std::vector<std::vector<uint32_t>>> cutAtWindows(const std::vector<std::vector<std::string>>& groups, uint32_t window) {
        std::vector<uint32_t> wfs{0}, len, bases;
        std::vector<uint64_t> off, cut_off{0};
        for (const auto& group : groups) {
            for (const auto& s : group) {
                const uint64_t words = (s.size() + 15) / 16;
                off.push_back(bases.size());
                len.push_back((uint32_t)s.size());
                bases.resize(bases.size() + words);
                if (words && cw_pack_sequence(s.data(), (uint32_t)s.size(), bases.data() + off.back(), words) < 0)
                    throw std::runtime_error("consent_amd: cw_pack_sequence failed");
                cut_off.push_back(cut_off.back() + (&s == &group.front() || window == 0 ? 0u : CW_SW_CUTS((uint32_t)group.front().size(), window)));
            }
            wfs.push_back((uint32_t)len.size());
        }
        bases.push_back(0);
        std::vector<int32_t> rows(len.size() * CW_SW_ROW + 1);
        std::vector<uint32_t> words(cut_off.back() + 1);
        cw_batch b{(uint32_t)groups.size(), (uint32_t)len.size(), (uint64_t)bases.size() - 1, wfs.data(), len.data(), off.data(), bases.data()};
        cw_sw_cuts cuts{words.data(), cut_off.data(), window};
        const int rc = cw_sw_cut_run(eng_, &b, rows.data(), &cuts);
        if (rc != CW_OK && rc != CW_E_CAPACITY) throw std::runtime_error(std::string("consent_amd: cw_sw_cut_run: ") + cw_strerror(rc));
        std::vector<std::vector<std::vector<uint32_t>>> out(groups.size());
        for (size_t g = 0; g < groups.size(); ++g)
            for (uint32_t s = wfs[g]; s < wfs[g + 1]; ++s) out[g].emplace_back(words.begin() + cut_off[s], words.begin() + cut_off[s + 1]);
        return out;
    }

    /* Both strands (cw_strand_run, cw_revcomp): every group with the members that are the reverse complement of the group's first sequence turned round, so
       that alignToFirst and cutAtWindows see them in its orientation; strands, when given, receives [g][m], the CW_STRAND_* value of member m of group g
       ([g][0] is CW_STRAND_IS_REF).  k = 0: CW_STRAND_K.  Positions computed from a turned member count from its other end.  (N packs as T: a turned member
       reads A where the original had N.) */
    std::vector<std::vector<std::string>> orientToFirst(const std::vector<std::vector<std::string>>& groups, uint32_t k = 0,
                                                        std::vector<std::vector<uint8_t>>* strands = nullptr) {
        std::vector<uint32_t> wfs{0}, len, bases;
        std::vector<uint64_t> off;
        for (const auto& group : groups) {
            for (const auto& s : group) {
                const uint64_t words = (s.size() + 15) / 16;
                off.push_back(bases.size());
                len.push_back((uint32_t)s.size());
                bases.resize(bases.size() + words);
                if (words && cw_pack_sequence(s.data(), (uint32_t)s.size(), bases.data() + off.back(), words) < 0)
                    throw std::runtime_error("consent_amd: cw_pack_sequence failed");
            }
            wfs.push_back((uint32_t)len.size());
        }
        bases.push_back(0);
        std::vector<uint8_t> strand(len.size() + 1);
        std::vector<uint32_t> turned(bases.size());
        cw_batch b{(uint32_t)groups.size(), (uint32_t)len.size(), (uint64_t)bases.size() - 1, wfs.data(), len.data(), off.data(), bases.data()};
        cw_strands votes{strand.data(), nullptr, k};
        int rc = cw_strand_run(eng_, &b, &votes);
        if (rc != CW_OK) throw std::runtime_error(std::string("consent_amd: cw_strand_run: ") + cw_strerror(rc));
        if ((rc = cw_revcomp(eng_, &b, strand.data(), turned.data())) != CW_OK) throw std::runtime_error(std::string("consent_amd: cw_revcomp: ") + cw_strerror(rc));
        std::vector<std::vector<std::string>> out(groups.size());
        if (strands) strands->assign(groups.size(), {});
        for (size_t g = 0; g < groups.size(); ++g)
            for (uint32_t s = wfs[g]; s < wfs[g + 1]; ++s) {
                if (strands) (*strands)[g].push_back(strand[s]);
                if (strand[s] != CW_STRAND_REV) { out[g].push_back(groups[g][s - wfs[g]]); continue; }
                std::string t(len[s], 'A');
                for (uint32_t j = 0; j < len[s]; ++j) t[j] = "ACGT"[(turned[off[s] + (j >> 4)] >> (30 - 2 * (j & 15))) & 3u];
                out[g].push_back(t);
            }
        return out;
    }

  private:
    cw_engine* eng_ = nullptr;
    unsigned solid_;
};

} // namespace consent_amd
#endif
