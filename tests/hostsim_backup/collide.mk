# TEST HARNESS build: the sixteen-lane backup's collision cancel (dev_backup16.h) compiled for the CPU as a stand-alone
# program, plain and under AddressSanitizer and UBSan (see collide_sim.cpp header). make -f collide.mk
CXX ?= g++
CXXFLAGS ?= -O2 -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wextra -Wno-unknown-pragmas
SANFLAGS ?= -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wextra -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all
SRC = ../../alpharat_amd/csrc
HDRS = $(SRC)/dev_backup16.h $(SRC)/dev_search.h $(SRC)/dev_engine.h $(SRC)/dev_rng.h
all: collide_sim collide_sim_san
collide_sim: collide_sim.cpp $(HDRS)
	$(CXX) $(CXXFLAGS) -o $@ collide_sim.cpp
collide_sim_san: collide_sim.cpp $(HDRS)
	$(CXX) $(SANFLAGS) -o $@ collide_sim.cpp
clean:
	rm -f collide_sim collide_sim_san
