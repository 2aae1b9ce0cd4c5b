// sw_pssm_read.cpp -- the reader and the writer of PSI-BLAST's ASCII PSSM (sw_read_pssm, sw_write_pssm; include/swhip.h).  Plain C++ that needs nothing of the
// library but the header and the error text: a stand-alone program can compile this file alone (tests/pssm_read_driver.cpp does,
// under the address and undefined-behaviour sanitizers).
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/swhip.h"

namespace swh {   // sw_host.cpp
void set_err(const char* fmt, ...);
}

extern "C" {

// PSI-BLAST's ASCII PSSM (include/swhip.h states the rules).  The file is read whole and cut into lines and tokens, as sw_read_submat
// does; every index below is into a std::string or std::vector of this function, and the outputs are written under `cap` and 256.
int sw_read_pssm(const char* path, char* letters_out, int32_t* nletters, int8_t* pssm, int64_t cap, int64_t* ncols) {
    if (!path || !letters_out || !nletters || !ncols || (pssm && cap < 0)) { swh::set_err("sw_read_pssm: bad argument"); return SW_EINVAL; }
    FILE* f = fopen(path, "rb");
    if (!f) { swh::set_err("sw_read_pssm: cannot open %s", path); return SW_EINVAL; }
    std::string text;
    char buf[1 << 14];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const bool err = ferror(f) != 0;
    fclose(f);
    if (err) { swh::set_err("sw_read_pssm: read error on %s", path); return SW_EINVAL; }
    std::string letters;             // the header's letters, in order
    std::vector<int8_t> cols;        // columns read x n
    int64_t n_cols = 0;
    int lineno = 0;
    for (size_t pos = 0; pos < text.size();) {
        size_t end = text.find_first_of("\r\n", pos);
        if (end == std::string::npos) end = text.size();
        std::vector<std::string> tok;
        for (size_t i = pos; i < end;) {
            while (i < end && (text[i] == ' ' || text[i] == '\t')) ++i;
            size_t j = i;
            while (j < end && text[j] != ' ' && text[j] != '\t') ++j;
            if (j > i) tok.push_back(text.substr(i, j - i));
            i = j;
        }
        pos = end + 1;
        if (end + 1 < text.size() && text[end] == '\r' && text[end + 1] == '\n') ++pos;   // CRLF is ONE line end, not a line and an empty line
        ++lineno;
        if (letters.empty()) {     // before the header: the first line whose tokens are all single letters
            bool all = !tok.empty();
            for (const std::string& t : tok) all = all && t.size() == 1 && ((t[0] >= 'A' && t[0] <= 'Z') || (t[0] >= 'a' && t[0] <= 'z') || t[0] == '*');
            if (!all) continue;
            for (const std::string& t : tok) {
                if (letters.find(t[0]) != std::string::npos) {
                    if (t[0] == letters[0]) break;       // the alphabet's second printing begins
                    swh::set_err("sw_read_pssm: %s line %d: letter '%c' is listed twice", path, lineno, t[0]);
                    return SW_EINVAL;
                }
                letters.push_back(t[0]);
            }
            continue;
        }
        // a column: position, residue letter, n integers; the first other line behind a column ends the table
        char* endp = nullptr;
        bool is_column = !tok.empty();
        if (is_column) {
            (void)strtol(tok[0].c_str(), &endp, 10);
            is_column = endp != tok[0].c_str() && !*endp;
        }
        if (!is_column) {
            if (n_cols > 0) break;
            continue;
        }
        const size_t n = letters.size();
        if (tok.size() < n + 2 || tok[1].size() != 1) {
            swh::set_err("sw_read_pssm: %s line %d: a column needs a position, a residue letter and %zu entries", path, lineno, n);
            return SW_EINVAL;
        }
        for (size_t i = 2; i < n + 2; ++i) {
            const long v = strtol(tok[i].c_str(), &endp, 10);
            if (endp == tok[i].c_str() || *endp) { swh::set_err("sw_read_pssm: %s line %d: '%s' is not an integer", path, lineno, tok[i].c_str()); return SW_EINVAL; }
            if (v < -128 || v > 127) { swh::set_err("sw_read_pssm: %s line %d: entry %ld does not fit int8", path, lineno, v); return SW_EINVAL; }
            cols.push_back((int8_t)v);
        }
        ++n_cols;
    }
    if (letters.empty()) { swh::set_err("sw_read_pssm: %s has no header line", path); return SW_EINVAL; }
    if (n_cols == 0) { swh::set_err("sw_read_pssm: %s has no column", path); return SW_EINVAL; }
    if (pssm && (int64_t)cols.size() > cap) { swh::set_err("sw_read_pssm: buffer too small (%zu bytes, cap = %lld)", cols.size(), (long long)cap); return SW_EINVAL; }
    std::copy(letters.begin(), letters.end(), letters_out);   // at most 53 distinct letters pass the header's test: inside 256
    *nletters = (int32_t)letters.size();
    *ncols = n_cols;
    if (pssm) std::copy(cols.begin(), cols.end(), pssm);
    return SW_OK;
}

// The writer of the same layout: a title line, the alphabet twice, per column its position, its residue, the scores and as many zero
// percentages, a blank line.  The contract is the reader's: only letters its header test accepts can be written.
int sw_write_pssm(const char* path, const char* letters, int32_t nletters, const int8_t* pssm, int64_t ncols, const char* consensus) {
    if (!path || !letters || !pssm) { swh::set_err("sw_write_pssm: NULL pointer"); return SW_EINVAL; }
    if (nletters < 1 || nletters > 256) { swh::set_err("sw_write_pssm: nletters = %d is out of range 1..256", nletters); return SW_EINVAL; }
    if (ncols < 1) { swh::set_err("sw_write_pssm: ncols = %lld: a file needs a column", (long long)ncols); return SW_EINVAL; }
    bool seen[256] = {};
    for (int k = 0; k < nletters; ++k) {
        const unsigned char b = (unsigned char)letters[k];
        if (!((b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || b == '*')) {
            swh::set_err("sw_write_pssm: letter 0x%02x cannot stand in the header of an ASCII PSSM (A-Z, a-z and '*' can)", b);
            return SW_EINVAL;
        }
        if (seen[b]) { swh::set_err("sw_write_pssm: letter '%c' is listed twice", b); return SW_EINVAL; }
        seen[b] = true;
    }
    if (consensus)
        for (int64_t g = 0; g < ncols; ++g)
            if ((unsigned char)consensus[g] <= ' ' || (unsigned char)consensus[g] > '~') {
                swh::set_err("sw_write_pssm: consensus byte 0x%02x of column %lld is not a printable character", (unsigned char)consensus[g], (long long)g);
                return SW_EINVAL;
            }
    std::string text = "\nLast position-specific scoring matrix computed, weighted observed percentages rounded down\n         ";
    for (int rep = 0; rep < 2; ++rep)
        for (int k = 0; k < nletters; ++k) { text += "   "; text += letters[k]; }
    text += '\n';
    char num[32];
    for (int64_t g = 0; g < ncols; ++g) {
        snprintf(num, sizeof num, "%5lld %c  ", (long long)(g + 1), consensus ? consensus[g] : 'X');
        text += num;
        for (int k = 0; k < nletters; ++k) { snprintf(num, sizeof num, " %3d", (int)pssm[g * nletters + k]); text += num; }
        for (int k = 0; k < nletters; ++k) text += "   0";
        text += '\n';
    }
    text += '\n';
    FILE* f = fopen(path, "wb");
    if (!f) { swh::set_err("sw_write_pssm: cannot open %s for writing", path); return SW_EINVAL; }
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) { swh::set_err("sw_write_pssm: write error on %s", path); return SW_EINVAL; }
    return SW_OK;
}

}  // extern "C"
